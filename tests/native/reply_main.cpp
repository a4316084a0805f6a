// The reply text rule (pbft_amd/csrc/reply_core.h), the host encoder and decoder (pbft_wire_encode_replies,
// pbft_wire_decode_reply, pbft_reply_digests; pbft_amd/csrc/host/wire.cpp) and the replica's reply path
// (pbft_replica_reply under a replier override; host/replica.cpp) as a stand-alone program, for AddressSanitizer +
// UndefinedBehaviorSanitizer (tests/test_reply.py).  A seeded loop of random results -- canonical ones and ones with
// escapes, non-ASCII bytes and too many bytes -- each batch in heap buffers of exactly its size: the results back to back
// with no slack, the output exactly the queried length, every text handed to the matcher in a buffer of exactly its
// length, so that a read or a write of one byte outside is a sanitizer report.  Every text is (1) compared with the
// core's writer run on its own where the result is canonical, (2) matched by pbft_wire_decode_reply, whose PBFT_RH_OK
// must coincide with PBFT_REPLY_OK and whose fields must be the inputs, and (3) mutated at a random byte and matched
// again (any answer, no report).  The replica is linked without the GPU library: the verifier entry points it names are
// stubs that report no device.
//   reply_main [rounds]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/pbft_replica.h"
#include "../../include/pbft_wire.h"
#include "../../pbft_amd/csrc/reply_core.h"

using namespace pbft;

static_assert(RP_ST_OK == PBFT_REPLY_OK && RP_ST_GENERAL == PBFT_REPLY_GENERAL && RP_RH_OK == PBFT_RH_OK &&
                  RP_RESULT_MAX == PBFT_REPLY_RESULT_MAX && RP_PEER_ID_B58 == PBFT_REPLY_PEER_ID_CHARS,
              "the core's values are the header's");

// ---- what replica.cpp links against from the GPU library: never reached without a context ----
extern "C" {
#define NODEV(name, ...) \
  int name(__VA_ARGS__) { return PBFT_ENODEV; }
NODEV(pbft_verify_ctx_clone, pbft_ctx*, pbft_ctx**)
NODEV(pbft_verify_ctx_destroy, pbft_ctx*)
NODEV(pbft_digest_blake2b512, pbft_ctx*, const uint8_t*, const uint64_t*, const uint32_t*, uint64_t, uint8_t*)
NODEV(pbft_verify_votes_stage, pbft_ctx*, uint64_t, uint32_t, pbft_votes_staging*)
NODEV(pbft_verify_votes_submit, pbft_ctx*, uint64_t, uint32_t, uint64_t*)
NODEV(pbft_verify_votes_submit_begin, pbft_ctx*, uint64_t, uint32_t, uint64_t*)
NODEV(pbft_verify_votes_submit_rows, pbft_ctx*, uint64_t)
NODEV(pbft_verify_votes_submit_host, pbft_ctx*, const uint8_t*, uint64_t, const uint8_t*, uint32_t, uint64_t*)
NODEV(pbft_verify_votes_open, pbft_ctx*, uint64_t, uint32_t, uint64_t*)
NODEV(pbft_verify_votes_piece, pbft_ctx*, const uint8_t*, uint64_t, uint64_t, const uint8_t*, uint32_t, uint32_t)
NODEV(pbft_verify_votes_close, pbft_ctx*, uint64_t)
NODEV(pbft_verify_poll_rows, pbft_ctx*, uint64_t*)
NODEV(pbft_verify_poll, pbft_ctx*)
NODEV(pbft_verify_wait, pbft_ctx*)
NODEV(pbft_verify_update_keys, pbft_ctx*, const uint32_t*, const uint8_t*, uint32_t, uint8_t*)
NODEV(pbft_verify_revoke_keys, pbft_ctx*, const uint32_t*, uint32_t)
NODEV(pbft_verify_key_set_id, pbft_ctx*, uint64_t*)
NODEV(pbft_host_alloc, pbft_ctx*, size_t, void**)
NODEV(pbft_host_free, pbft_ctx*, void*)
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}
static uint64_t rnd_width() {  // a u64 of a random decimal width
  const uint64_t v = rnd() >> (rnd() % 64);
  return rnd() % 8 == 0 ? ~0ull - rnd() % 3 : v;
}
static uint8_t rnd_canon() {
  for (;;) {
    const uint8_t c = (uint8_t)(0x20 + rnd() % 0x5F);
    if (pr_alphabet(c)) return c;
  }
}

#define CHECK(x)                                                          \
  do {                                                                    \
    if (!(x)) {                                                           \
      fprintf(stderr, "reply_main: %s failed (line %d)\n", #x, __LINE__); \
      return 1;                                                           \
    }                                                                     \
  } while (0)

// A batch of random results in exactly-sized heap buffers.
struct Batch {
  uint64_t N = 0;
  std::vector<uint64_t> off, ts;
  std::vector<uint32_t> len;
  uint8_t* results = nullptr;  // exactly results_bytes
  uint64_t results_bytes = 0;
  uint8_t* clients = nullptr;  // exactly 64 * N
  explicit Batch(uint64_t n) : N(n), off(n), ts(n), len(n) {
    static const uint32_t lens[] = {0, 1, 2, 13, 63, 64, 65, 191, 192, 193, 1000, 3071, 3072, 3073, 5000};
    static const uint8_t odd[] = {'"', '\\', 0x1F, 0x7F, '\n', 0x00, 0x80, 0xFF};
    std::vector<uint8_t> raw;
    for (uint64_t i = 0; i < N; ++i) {
      off[i] = raw.size();
      len[i] = lens[rnd() % (sizeof lens / sizeof *lens)];
      ts[i] = rnd_width();
      for (uint32_t k = 0; k < len[i]; ++k) raw.push_back(rnd_canon());
      if (len[i] && rnd() % 3 == 0) raw[off[i] + (rnd() % 3 == 0 ? 0 : rnd() % 2 ? len[i] - 1 : len[i] / 2)] = odd[rnd() % sizeof odd];
      if (len[i] >= 2 && rnd() % 7 == 0) {  // a two-byte UTF-8 character
        const size_t at = off[i] + (rnd() % 2 ? 0 : len[i] - 2);
        raw[at] = 0xC3, raw[at + 1] = 0xA9;
      }
    }
    results_bytes = raw.size();
    results = (uint8_t*)malloc(raw.size() ? raw.size() : 1);
    if (!raw.empty()) memcpy(results, raw.data(), raw.size());
    clients = (uint8_t*)malloc(N ? 64 * N : 1);
    static const uint32_t clens[] = {14, 1, 63, 0, 64, 20};
    for (uint64_t i = 0; i < N; ++i) {
      const uint32_t cl = clens[rnd() % 6];
      for (uint32_t k = 0; k < 64; ++k) clients[64 * i + k] = k < cl ? rnd_canon() : (rnd() % 2 ? 0 : (uint8_t)rnd());
      if (cl < 64) clients[64 * i + cl] = 0;  // bytes behind the first NUL: junk
    }
  }
  ~Batch() {
    free(results);
    free(clients);
  }
};

static int match_exact(const uint8_t* text, size_t n, pbft_reply_head* h) {  // a buffer of exactly the text
  uint8_t* t = (uint8_t*)malloc(n ? n : 1);
  if (n) memcpy(t, text, n);
  const int rc = pbft_wire_decode_reply(t, n, h);
  free(t);
  return rc;
}

// The replier override: fixed signature bytes and a fixed PeerId text through the host encoder.
static const char PEER[] = "12D3KooWAnswerMainAnswerMainAnswerMainAnswerMainAnsw";
static_assert(sizeof PEER == RP_PEER_ID_B58 + 1, "52 characters");
static uint64_t g_replier_calls = 0;
static int replier(void*, const uint8_t* results, uint64_t, const uint64_t* res_off, const uint32_t* res_len,
                   const uint64_t* timestamp, const char*, uint64_t view, uint64_t n, uint32_t replica, uint8_t* out,
                   size_t cap, size_t* len) {
  ++g_replier_calls;
  std::vector<uint8_t> sigs(64 * n, 0x5A);
  return pbft_wire_encode_replies(n, view, timestamp, results, res_off, res_len, replica, PEER, sigs.data(), out, cap,
                                  len, nullptr, nullptr);
}
static int accept_all(void*, const uint8_t*, const uint8_t*, const uint16_t*, const uint8_t*, uint32_t, uint32_t,
                      uint64_t N, uint64_t* out) {
  for (uint64_t w = 0; w < (N + 63) / 64; ++w) out[w] = ~0ull;
  return 0;
}
static int fake_digest(void*, const uint8_t* op, uint32_t n, uint8_t out[64]) {
  memset(out, 0x11, 64);
  for (uint32_t i = 0; i < n; ++i) out[i % 64] ^= op[i];
  return 0;
}

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 200;
  uint64_t replies = 0, canon = 0, through = 0;

  // ---- the encoder, the decoder and the digests ----
  for (int round = 0; round < rounds; ++round) {
    Batch b(rnd() % 9);
    const uint64_t N = b.N, view = rnd_width();
    const uint32_t replica = (uint32_t)(rnd() % 65536);
    uint8_t* sig = (uint8_t*)malloc(N ? 64 * N : 1);
    for (uint64_t k = 0; k < 64 * N; ++k) sig[k] = (uint8_t)rnd();
    char* pid = (char*)malloc(RP_PEER_ID_B58);  // exactly the 52 characters, no NUL
    memcpy(pid, PEER, RP_PEER_ID_B58);

    size_t need = 0;
    CHECK(pbft_wire_encode_replies(N, view, b.ts.data(), b.results, b.off.data(), b.len.data(), replica, nullptr, nullptr,
                                   nullptr, 0, &need, nullptr, nullptr) == 0);
    uint8_t* out = (uint8_t*)malloc(need ? need : 1);  // exactly the stream
    uint64_t* roff = (uint64_t*)malloc(8 * (N + 1));
    uint8_t* st = (uint8_t*)malloc(N ? N : 1);
    size_t got = 0;
    CHECK(pbft_wire_encode_replies(N, view, b.ts.data(), b.results, b.off.data(), b.len.data(), replica, pid, sig, out,
                                   need, &got, roff, st) == 0);
    CHECK(got == need && roff[0] == 0 && roff[N] == need);
    if (need) {  // one byte short: refused, the length still reported
      size_t l2 = 0;
      uint8_t* shorter = (uint8_t*)malloc(need - 1 ? need - 1 : 1);
      CHECK(pbft_wire_encode_replies(N, view, b.ts.data(), b.results, b.off.data(), b.len.data(), replica, pid, sig,
                                     shorter, need - 1, &l2, nullptr, nullptr) == PBFT_EINVAL);
      CHECK(l2 == need);
      free(shorter);
    }
    uint8_t* dig = (uint8_t*)malloc(N ? 64 * N : 1);
    CHECK(pbft_reply_digests(N, (const char*)b.clients, b.results, b.results_bytes, b.off.data(), b.len.data(), dig) == 0);
    for (uint64_t i = 0; i < N; ++i) {
      const size_t tl = (size_t)(roff[i + 1] - roff[i]);
      const uint8_t* tx = out + roff[i];
      const uint8_t* res = b.results + b.off[i];
      const bool can = rp_canonical(res, b.len[i]);
      CHECK(st[i] == (can ? PBFT_REPLY_OK : PBFT_REPLY_GENERAL));
      if (can) {  // the core's writer on its own
        CHECK(tl == rp_text_len(view, b.ts[i], replica, b.len[i]));
        uint8_t* mine = (uint8_t*)malloc(tl);
        uint32_t sw[16];
        memcpy(sw, sig + 64 * i, 64);
        auto put = [mine](uint32_t pos, uint8_t v) { mine[pos] = v; };
        CHECK(rp_write_text(put, view, b.ts[i], (const uint8_t*)pid, res, b.len[i], replica, sw) == tl);
        CHECK(memcmp(mine, tx, tl) == 0);
        free(mine);
        ++canon;
      }
      pbft_reply_head h;
      CHECK(match_exact(tx, tl, &h) == 0);
      CHECK((h.status == PBFT_RH_OK) == can);
      if (can) {
        CHECK(h.view == view && h.timestamp == b.ts[i] && h.replica == replica && h.result_len == b.len[i]);
        CHECK(b.len[i] == 0 || memcmp(tx + h.result_off, res, b.len[i]) == 0);
        CHECK(memcmp(h.peer_id, pid, RP_PEER_ID_B58) == 0 && memcmp(h.sig, sig + 64 * i, 64) == 0);
      }
      if (tl) {  // a mutation and a truncation: any answer
        uint8_t* mut = (uint8_t*)malloc(tl);
        memcpy(mut, tx, tl);
        mut[rnd() % tl] = (uint8_t)rnd();
        CHECK(pbft_wire_decode_reply(mut, tl, &h) == 0);
        free(mut);
        CHECK(match_exact(tx, rnd() % tl, &h) == 0);
        CHECK(h.status == PBFT_RH_NONE);
      }
      // the digest does not depend on what stands behind the client's NUL
      uint8_t c2[64], d2[64];
      rp_client_norm(c2, b.clients + 64 * i);
      const uint64_t zero = 0;
      uint8_t* r2 = (uint8_t*)malloc(b.len[i] ? b.len[i] : 1);
      if (b.len[i]) memcpy(r2, res, b.len[i]);
      CHECK(pbft_reply_digests(1, (const char*)c2, r2, b.len[i], &zero, &b.len[i], d2) == 0);
      CHECK(memcmp(d2, dig + 64 * i, 64) == 0);
      free(r2);
      ++replies;
    }
    free(dig);
    free(st);
    free(roff);
    free(out);
    free(pid);
    free(sig);
  }

  // ---- the PeerId text ----
  for (int k = 0; k < 200; ++k) {
    uint8_t A[32], back[32];
    for (int j = 0; j < 32; ++j) A[j] = k == 0 ? 0x00 : k == 1 ? 0xFF : (uint8_t)rnd();
    char* text = (char*)malloc(RP_PEER_ID_B58);
    CHECK(pbft_peer_id_b58_from_key(A, text) == 0);
    CHECK(pbft_key_from_peer_id_b58(text, RP_PEER_ID_B58, back) == 0 && memcmp(A, back, 32) == 0);
    free(text);
  }

  // ---- the replica: seqs 1 .. 8 committed-local under a verifier that accepts everything ----
  {
    const uint32_t n_rep = 4, self = 2;
    const uint64_t view = 1, n_seq = 8;
    std::vector<uint8_t> keys(32 * n_rep);
    for (size_t i = 0; i < keys.size(); ++i) keys[i] = (uint8_t)(i * 37 + i / 32);
    pbft_replica* r = nullptr;
    CHECK(pbft_replica_create(nullptr, n_rep, self, keys.data(), &r) == 0);
    CHECK(pbft_replica_set_verifier(r, accept_all, nullptr) == 0);
    CHECK(pbft_replica_set_digest_fn(r, fake_digest, nullptr) == 0);
    uint8_t sigz[64] = {0};
    std::vector<pbft_round_event> ev(256);
    uint32_t ne = 0;
    for (uint64_t q = 1; q <= n_seq; ++q) {
      const uint8_t op[3] = {'o', 'p', (uint8_t)q};
      uint8_t d[64];
      fake_digest(nullptr, op, 3, d);
      CHECK(pbft_replica_on_pre_prepare(r, (uint32_t)(view % n_rep), view, q, op, 3, d, sigz, nullptr) == 1);
      for (uint8_t kind = PBFT_KIND_PREPARE; kind <= PBFT_KIND_COMMIT; ++kind)
        for (uint32_t s = 0; s < n_rep; ++s) CHECK(pbft_replica_push(r, kind, view, q, d, s, sigz) >= 0);
    }
    for (int k = 0; k < 4; ++k) CHECK(pbft_replica_flush(r, 1, ev.data(), (uint32_t)ev.size(), &ne) == 0);
    for (uint64_t q = 1; q <= n_seq; ++q) CHECK(pbft_replica_committed_local(r, view, q) == 1);
    CHECK(pbft_replica_committed_local(r, view, n_seq + 1) == 0);
    CHECK(pbft_replica_set_replier(r, replier, nullptr) == 0);

    for (int round = 0; round < rounds; ++round) {
      Batch b(rnd() % 9);
      const uint64_t N = b.N;
      std::vector<uint64_t> seq(N);
      for (uint64_t i = 0; i < N; ++i) {
        seq[i] = 1 + rnd() % (n_seq + 2);   // now and then an uncommitted one
        b.ts[i] = 1 + rnd() % 40;           // now and then a stale one
      }
      CHECK(pbft_replica_set_last_timestamp(r, rnd() % 10) == 0);
      uint64_t before = 0, after = 0, n_made = 0, q_made = 0;
      CHECK(pbft_replica_last_timestamp(r, &before) == 0);
      // the model: the exactly-once rule over the committed entries
      std::vector<uint8_t> want(N);
      uint64_t last = before;
      for (uint64_t i = 0; i < N; ++i) {
        if (seq[i] > n_seq) want[i] = PBFT_REPLY_NOT_COMMITTED;
        else if (b.ts[i] <= last) want[i] = PBFT_REPLY_STALE;
        else {
          want[i] = rp_canonical(b.results + b.off[i], b.len[i]) ? PBFT_REPLY_OK : PBFT_REPLY_GENERAL;
          last = b.ts[i];
        }
      }
      size_t need = 0, got = 0;
      uint64_t* roff = (uint64_t*)malloc(8 * (N + 1));
      uint8_t* st = (uint8_t*)malloc(N ? N : 1);
      const uint64_t calls0 = g_replier_calls;
      CHECK(pbft_replica_reply(r, N, seq.data(), b.ts.data(), (const char*)b.clients, b.results, b.results_bytes,
                               b.off.data(), b.len.data(), 0, nullptr, 0, &need, roff, st, &q_made) == 0);
      CHECK(pbft_replica_last_timestamp(r, &after) == 0 && after == before && g_replier_calls == calls0);
      if (need) {  // a short cap changes nothing
        uint8_t* shorter = (uint8_t*)malloc(need - 1 ? need - 1 : 1);
        CHECK(pbft_replica_reply(r, N, seq.data(), b.ts.data(), (const char*)b.clients, b.results, b.results_bytes,
                                 b.off.data(), b.len.data(), 0, shorter, need - 1, &got, nullptr, nullptr,
                                 nullptr) == PBFT_EINVAL);
        CHECK(got == need && pbft_replica_last_timestamp(r, &after) == 0 && after == before);
        free(shorter);
      }
      uint8_t* out = (uint8_t*)malloc(need ? need : 1);  // exactly the stream
      CHECK(pbft_replica_reply(r, N, seq.data(), b.ts.data(), (const char*)b.clients, b.results, b.results_bytes,
                               b.off.data(), b.len.data(), 0, out, need, &got, roff, st, &n_made) == 0);
      CHECK(got == need && n_made == q_made && roff[N] == need);
      CHECK(pbft_replica_last_timestamp(r, &after) == 0 && after == last);
      for (uint64_t i = 0; i < N; ++i) {
        CHECK(st[i] == want[i]);
        const size_t tl = (size_t)(roff[i + 1] - roff[i]);
        CHECK((tl != 0) == (want[i] <= PBFT_REPLY_GENERAL));
        if (want[i] == PBFT_REPLY_OK) {
          pbft_reply_head h;
          CHECK(match_exact(out + roff[i], tl, &h) == 0 && h.status == PBFT_RH_OK);
          CHECK(h.view == view && h.timestamp == b.ts[i] && h.replica == self && h.result_len == b.len[i]);
          ++through;
        }
      }
      free(out);
      free(st);
      free(roff);
    }
    pbft_replica_reply_stats s;
    CHECK(pbft_replica_get_reply_stats(r, &s) == 0 && s.calls == (uint64_t)rounds && s.replied >= through);
    CHECK(pbft_replica_destroy(r) == 0);
  }
  printf("reply host run ok: %llu replies, %llu canonical, %llu through the replica\n", (unsigned long long)replies,
         (unsigned long long)canon, (unsigned long long)through);
  return 0;
}
