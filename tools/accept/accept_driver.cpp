// The host loops of tools/accept_probe.py's leg (a*): what a client had to write itself before pbft_accept_replies,
// through the entry points that existed then, as plain C loops (no per-reply call overhead from Python).  Built by the
// probe into tools/accept/libaccept_driver.so, linked against the in-tree library.
#include <stdint.h>
#include <string.h>

#include "../../include/pbft_replica.h"
#include "../../include/pbft_wire.h"

extern "C" {

// Step 1: pbft_wire_decode_reply per text, the signer's claim against the PeerId table [n_keys][52], and the columns the
// later steps take: the result's span (absolute), the client's 64-byte field per reply, R, S, the key index (0xFFFF: the
// reply is dropped) and view / timestamp.  Returns the number of replies kept.
uint64_t accept_driver_decode(const uint8_t* texts, const uint64_t* off, const uint32_t* len, uint64_t n,
                              const char* pid_table, uint32_t n_keys, const uint32_t* client_idx, const char* clients,
                              uint32_t n_clients, uint64_t* res_off, uint32_t* res_len, char* client_rows, uint8_t* R,
                              uint8_t* S, uint16_t* key, uint64_t* view, uint64_t* ts) {
  uint64_t kept = 0;
  for (uint64_t i = 0; i < n; ++i) {
    pbft_reply_head h;
    key[i] = 0xFFFF;
    res_off[i] = 0;
    res_len[i] = 0;
    view[i] = ts[i] = 0;
    memset(R + 32 * i, 0, 32);
    memset(S + 32 * i, 0, 32);
    memset(client_rows + 64 * i, 0, 64);
    if (pbft_wire_decode_reply(texts + off[i], len[i], &h) != 0 || h.status != PBFT_RH_OK) continue;
    if (h.replica >= n_keys || memcmp(h.peer_id, pid_table + 52 * (size_t)h.replica, 52) != 0) continue;
    const uint32_t ci = client_idx ? client_idx[i] : 0;
    if (ci >= n_clients) continue;
    res_off[i] = off[i] + h.result_off;
    res_len[i] = h.result_len;
    memcpy(client_rows + 64 * i, clients + 64 * (size_t)ci, 64);
    memcpy(R + 32 * i, h.sig, 32);
    memcpy(S + 32 * i, h.sig + 32, 32);
    key[i] = (uint16_t)h.replica;
    view[i] = h.view;
    ts[i] = h.timestamp;
    ++kept;
  }
  return kept;
}

// Step 3's envelopes: pbft_reply_envelope per kept reply (zeros for a dropped one), stride 85.
void accept_driver_envelopes(uint64_t n, const uint16_t* key, const uint64_t* view, const uint64_t* ts,
                             const uint8_t* digests, uint8_t* env) {
  for (uint64_t i = 0; i < n; ++i) {
    if (key[i] == 0xFFFF) memset(env + 85 * i, 0, 85);
    else pbft_reply_envelope(env + 85 * i, view[i], ts[i], digests + 64 * i);
  }
}

// Step 6: the f + 1 comparison and the first-valid search over what came back.
void accept_driver_certify(uint64_t n, const uint64_t* bitmap, const uint32_t* env_idx, uint32_t n_env,
                           const uint32_t* count, uint32_t need, uint32_t* first, uint32_t* accepted) {
  for (uint32_t e = 0; e < n_env; ++e) {
    first[e] = 0xFFFFFFFFu;
    accepted[e] = count[e] >= need;
  }
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t e = env_idx[i];
    if (e < n_env && ((bitmap[i >> 6] >> (i & 63)) & 1) && first[e] == 0xFFFFFFFFu) first[e] = (uint32_t)i;
  }
}

}  // extern "C"
