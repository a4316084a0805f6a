// Stand-alone host run of the client's acceptance rule for AddressSanitizer + UBSan (tests/test_accept.py): the general
// reader pbft_wire_decode_reply_json and accept_core.h's host build over a corpus file, its truncations and its
// single-byte mutations, every text in a heap buffer of exactly its length.
//   accept_main <corpus>   corpus: 4 x 52 PeerId characters | 3 x 64 client bytes | { u32 client_idx, u32 len, text }*
// Checked on every text and variant: ac_match_frame + the alphabet test answer what rp_match answers, field for field;
// the general reader returns rp_match's fields wherever that one accepts and never reads outside the text; ac_decide's
// record is pbft_records_pack of the same signature, envelope and key index.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/pbft_replica.h"
#include "../../include/pbft_wire.h"
#include "../../pbft_amd/csrc/accept_core.h"

using namespace pbft;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

// What wire.cpp links against from replica.cpp (pbft_wire_decode_votes builds its rows' envelopes with it): the envelope
// itself, "PBFT" | kind | view LE | seq LE | digest.
extern "C" void pbft_envelope(uint8_t out[85], uint8_t kind, uint64_t view, uint64_t seq, const uint8_t digest[64]) {
  memcpy(out, "PBFT", 4);
  out[4] = kind;
  for (int j = 0; j < 8; ++j) {
    out[5 + j] = (uint8_t)(view >> (8 * j));
    out[13 + j] = (uint8_t)(seq >> (8 * j));
  }
  memcpy(out + 21, digest, 64);
}

static const uint32_t N_KEYS = 4, N_CLIENTS = 3;
static uint8_t g_pids[N_KEYS * 52];
static char g_clients[N_CLIENTS * 64];
static uint64_t n_canonical = 0, n_parsed = 0, n_variants = 0;

// One text (exactly n bytes on the heap): every reader against every other.  Returns through the counters.
static void run_text(const uint8_t* src, size_t n, uint32_t ci, bool count) {
  uint8_t* t = (uint8_t*)malloc(n ? n : 1);
  CHECK(t);
  if (n) memcpy(t, src, n);
  rp_head rh;
  const bool canon = rp_match(t, n, rh) == RP_RH_OK;
  // the two-ended matcher
  accept_frame f{};
  uint32_t sg[16];
  const ac_ptr_reader rd{t};
  const bool mine = ac_match_frame(rd, n, f, sg) && pr_all_alphabet(t + f.result_off, f.result_len);
  CHECK(mine == canon);
  if (canon) {
    CHECK(f.view == rh.view && f.timestamp == rh.timestamp && f.result_off == rh.result_off &&
          f.result_len == rh.result_len && f.replica == rh.replica);
    CHECK(memcmp(sg, rh.sig, 64) == 0 && memcmp(t + f.pid_off, rh.peer_id, 52) == 0);
  }
  // the general reader
  pbft_reply_head jh, ch;
  std::vector<char> arena(n + 1);
  const int rl = pbft_wire_decode_reply_json(t, n, &jh, arena.data(), n);
  CHECK(pbft_wire_decode_reply(t, n, &ch) == 0);
  if (canon) {
    CHECK(rl == (int)rh.result_len && memcmp(&jh, &ch, sizeof jh) == 0);
    CHECK(memcmp(arena.data(), t + rh.result_off, rh.result_len) == 0);
  } else if (rl >= 0) {
    CHECK(jh.status == PBFT_RH_GENERAL && (size_t)jh.result_off + jh.result_len <= n && (size_t)rl <= n);
    CHECK(jh.replica <= 65535);
  } else {
    const pbft_reply_head zero{};
    CHECK(memcmp(&jh, &zero, sizeof jh) == 0);
  }
  // the rule and the record
  accept_head h;
  uint32_t sig[16];
  const uint32_t st = ac_decide(t, n, g_pids, N_KEYS, ci, N_CLIENTS, h, sig);
  CHECK(h.status == st && (st == AC_EDEFER) == !canon);
  if (st == AC_OK) {
    uint8_t D[64], env[85], want[160];
    const uint64_t o = h.result_off;
    CHECK(pbft_reply_digests(1, g_clients + 64 * ci, t, n, &o, &h.result_len, D) == 0);
    uint32_t dw[16], rec[40];
    memcpy(dw, D, 64);
    ac_record(rec, sig, h.view, h.timestamp, dw, h.replica);
    pbft_envelope(env, PBFT_KIND_REPLY, h.view, h.timestamp, D);
    const uint16_t key = (uint16_t)h.replica;
    CHECK(pbft_records_pack((const uint8_t*)sig, (const uint8_t*)sig + 32, &key, env, 85, 1, want) == 0);
    CHECK(memcmp(rec, want, 160) == 0);
  } else {
    CHECK(h.view == 0 && h.timestamp == 0 && h.result_off == 0 && h.result_len == 0 && h.replica == 0);
    uint32_t rec[40];
    uint8_t want[160] = {0};
    ac_record_none(rec);
    want[150] = want[151] = 0xFF;
    CHECK(memcmp(rec, want, 160) == 0);
  }
  if (count) {
    n_canonical += canon;
    n_parsed += rl >= 0;
  } else {
    ++n_variants;
  }
  free(t);
}

int main(int argc, char** argv) {
  CHECK(argc == 2);
  FILE* fp = fopen(argv[1], "rb");
  CHECK(fp);
  std::vector<uint8_t> blob;
  uint8_t chunk[1 << 16];
  size_t got;
  while ((got = fread(chunk, 1, sizeof chunk, fp)) > 0) blob.insert(blob.end(), chunk, chunk + got);
  fclose(fp);
  CHECK(blob.size() >= sizeof g_pids + sizeof g_clients);
  memcpy(g_pids, blob.data(), sizeof g_pids);
  memcpy(g_clients, blob.data() + sizeof g_pids, sizeof g_clients);
  for (uint32_t c = 0; c < 256; ++c) CHECK(ac_b58_char(c) == rp_b58_char(c));

  uint64_t n_texts = 0;
  uint32_t lcg = 12345;
  auto rnd = [&]() { return lcg = lcg * 1664525u + 1013904223u, lcg >> 8; };
  size_t at = sizeof g_pids + sizeof g_clients;
  while (at < blob.size()) {
    CHECK(blob.size() - at >= 8);
    uint32_t ci, n;
    memcpy(&ci, blob.data() + at, 4);
    memcpy(&n, blob.data() + at + 4, 4);
    at += 8;
    CHECK(blob.size() - at >= n);
    const uint8_t* t = blob.data() + at;
    at += n;
    ++n_texts;
    run_text(t, n, ci, true);
    // truncations: every length of a short text, 96 lengths of a long one (its ends always)
    const bool small = n <= 640;
    for (uint32_t k = 0; k < (small ? n : 96u); ++k) {
      const uint32_t cut = small ? k : (k < 32 ? k : k < 64 ? n - 1 - (k - 32) : rnd() % n);
      run_text(t, cut, ci, false);
    }
    // single-byte mutations: every position of a short text (one bit, and a byte that matters to a parser), 160
    // positions of a long one (its head and tail always)
    std::vector<uint8_t> m(t, t + n);
    static const uint8_t special[] = {'"', '\\', ' ', '0', '}', 0x00, 0x80, 'A', ',', ':'};
    for (uint32_t k = 0; k < (small ? n : 160u); ++k) {
      const uint32_t pos = small ? k : (k < 64 ? k * 2 : k < 128 ? n - 1 - (k - 64) * 2 : rnd() % n);
      if (pos >= n) continue;
      const uint8_t keep = m[pos];
      m[pos] = keep ^ (uint8_t)(1u << (rnd() % 8));
      run_text(m.data(), n, ci, false);
      m[pos] = special[rnd() % sizeof special];
      run_text(m.data(), n, ci, false);
      m[pos] = keep;
    }
    // a client index out of range
    run_text(t, n, N_CLIENTS, false);
    run_text(t, n, 0xFFFFFFFFu, false);
  }
  printf("accept host run ok: %llu texts, %llu canonical, %llu parsed, %llu variants\n", (unsigned long long)n_texts,
         (unsigned long long)n_canonical, (unsigned long long)n_parsed, (unsigned long long)n_variants);
  return 0;
}
