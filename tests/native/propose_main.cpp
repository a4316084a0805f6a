// The proposal frame rule (pbft_amd/csrc/propose_core.h) and the host encoder (pbft_wire_encode_preprepares,
// pbft_amd/csrc/host/wire.cpp) as a stand-alone program, for AddressSanitizer + UndefinedBehaviorSanitizer
// (tests/test_propose.py).  A seeded loop of random requests -- canonical ones and ones with escapes, long operations,
// empty and unterminated clients -- each batch in heap buffers of exactly its size: the operations back to back with no
// slack, the output exactly the queried length, so that a read or a write of one byte outside is a sanitizer report.
// Every frame is then (1) compared with the core's writer run on its own into an exactly-sized buffer where the request
// is canonical, (2) parsed back by pbft_wire_decode_json, and (3) matched by the rule of pbft_wire_decode_preprepare (wire_pp_core.h), whose PBFT_PP_OK
// must coincide with PBFT_PROPOSE_OK and whose fields must be the inputs.
//   propose_main [rounds]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/pbft_wire.h"
#include "../../pbft_amd/csrc/propose_core.h"
#include "../../pbft_amd/csrc/wire_pp_core.h"

using namespace pbft;

static_assert(PR_OP_MAX == PP_OP_MAX && PR_CLIENT_MAX == PP_CLIENT_MAX && PR_BODY_MIN == PP_FRAME_MIN &&
                  PR_BODY_MAX == PP_FRAME_MAX, "the writer's limits are the matcher's");

// pbft_wire_decode_preprepare (wire_pp.hip, which is compiled with the kernels): the same rule, built here for the host
static int decode_preprepare(const uint8_t* body, size_t len, pbft_pp_head* out) {
  memset(out, 0, sizeof *out);
  if (len < PP_FRAME_MIN || len > PP_FRAME_MAX) return 0;
  const frame_mem_reader rd{body, 0, (uint32_t)len, 0xAA};
  pp_fields h;
  if (wire_pp_frame(rd, pp_byte_scan<frame_mem_reader>{rd}, 0, (uint32_t)len, h) != PP_ST_OK) return 0;
  out->view = h.view;
  out->seq = h.seq;
  out->timestamp = h.timestamp;
  out->op_off = h.op_off;
  out->op_len = h.op_len;
  out->replica = (uint16_t)h.replica;
  out->status = PBFT_PP_OK;
  memcpy(out->claimed, h.claimed, 64);
  memcpy(out->sig, h.sig, 64);
  pp_digest(out->computed, body, h.op_off, h.op_len);
  return 0;
}

// wire.cpp's vote decoder refers to pbft_envelope (host/replica.cpp, which is not linked here)
extern "C" void pbft_envelope(uint8_t out[85], uint8_t kind, uint64_t view, uint64_t seq, const uint8_t digest[64]) {
  memcpy(out, "PBFT", 4);
  out[4] = kind;
  for (int j = 0; j < 8; ++j) out[5 + j] = (uint8_t)(view >> (8 * j)), out[13 + j] = (uint8_t)(seq >> (8 * j));
  memcpy(out + 21, digest, 64);
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

#define CHECK(x)                                                        \
  do {                                                                  \
    if (!(x)) {                                                         \
      fprintf(stderr, "propose_main: %s failed (line %d)\n", #x, __LINE__); \
      return 1;                                                         \
    }                                                                   \
  } while (0)

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 200;
  static const uint32_t lens[] = {0, 1, 2, 13, 127, 128, 129, 1000, 3071, 3072, 3073, 5000};
  static const uint8_t odd[] = {'"', '\\', 0x1F, 0x7F, '\n', 0x00};
  uint64_t frames = 0, canon = 0;
  for (int round = 0; round < rounds; ++round) {
    const uint64_t N = rnd() % 9;
    const uint64_t view = rnd_width();
    uint64_t first = rnd_width();
    if (N && first + (N - 1) < first) first -= N;
    const uint32_t replica = (uint32_t)(rnd() % 65536);
    std::vector<uint64_t> off(N), ts(N);
    std::vector<uint32_t> ol(N);
    std::vector<uint8_t> raw;
    uint8_t* clients = (uint8_t*)malloc(N ? 64 * N : 1);
    for (uint64_t i = 0; i < N; ++i) {
      off[i] = raw.size();
      ol[i] = lens[rnd() % (sizeof lens / sizeof *lens)];
      ts[i] = rnd_width();
      for (uint32_t k = 0; k < ol[i]; ++k) raw.push_back(rnd_canon());
      if (ol[i] && rnd() % 3 == 0) raw[off[i] + (rnd() % 2 ? 0 : ol[i] - 1)] = odd[rnd() % sizeof odd];
      if (ol[i] >= 2 && rnd() % 7 == 0) {  // a two-byte UTF-8 character
        const size_t at = off[i] + (rnd() % 2 ? 0 : ol[i] - 2);
        raw[at] = 0xC3, raw[at + 1] = 0xA9;
      }
      static const uint32_t clens[] = {14, 1, 63, 0, 64, 20};
      const uint32_t cl = clens[rnd() % 6];
      memset(clients + 64 * i, 0, 64);
      for (uint32_t k = 0; k < cl; ++k) clients[64 * i + k] = rnd_canon();
      if (cl && rnd() % 9 == 0) clients[64 * i + rnd() % cl] = '"';
    }
    uint8_t* ops = (uint8_t*)malloc(raw.size() ? raw.size() : 1);  // exactly the operations
    if (!raw.empty()) memcpy(ops, raw.data(), raw.size());
    uint8_t* dig = (uint8_t*)malloc(N ? 64 * N : 1);
    uint8_t* sig = (uint8_t*)malloc(N ? 64 * N : 1);
    for (uint64_t k = 0; k < 64 * N; ++k) dig[k] = (uint8_t)rnd(), sig[k] = (uint8_t)rnd();

    size_t need = 0;
    CHECK(pbft_wire_encode_preprepares(N, view, first, ops, off.data(), ol.data(), ts.data(), (const char*)clients,
                                       replica, nullptr, nullptr, nullptr, 0, &need, nullptr, nullptr) == 0);
    uint8_t* out = (uint8_t*)malloc(need ? need : 1);  // exactly the stream
    uint64_t* foff = (uint64_t*)malloc(8 * (N + 1));
    uint8_t* st = (uint8_t*)malloc(N ? N : 1);
    size_t got = 0;
    CHECK(pbft_wire_encode_preprepares(N, view, first, ops, off.data(), ol.data(), ts.data(), (const char*)clients,
                                       replica, dig, sig, out, need, &got, foff, st) == 0);
    CHECK(got == need && foff[0] == 0 && foff[N] == need);
    if (need) {  // one byte short: refused, the length still reported
      size_t l2 = 0;
      uint8_t* shorter = (uint8_t*)malloc(need - 1 ? need - 1 : 1);
      CHECK(pbft_wire_encode_preprepares(N, view, first, ops, off.data(), ol.data(), ts.data(), (const char*)clients,
                                         replica, dig, sig, shorter, need - 1, &l2, nullptr, nullptr) == PBFT_EINVAL);
      CHECK(l2 == need);
      free(shorter);
    }
    for (uint64_t i = 0; i < N; ++i) {
      const size_t fl = (size_t)(foff[i + 1] - foff[i]);
      const uint8_t* fr = out + foff[i];
      uint64_t body = 0;
      size_t hn = 0;
      CHECK(pbft_uvi_decode(fr, fl, &body, &hn) == 0 && hn + body == fl);
      const uint8_t* cl = clients + 64 * i;
      const uint32_t cl_len = pr_client_len(cl);
      const bool can = pr_canonical(ops + off[i], ol[i], cl, cl_len);
      CHECK(st[i] == (can ? PBFT_PROPOSE_OK : PBFT_PROPOSE_GENERAL));
      if (can) {  // the core's writer on its own
        CHECK(fl == pr_frame_len(view, first + i, ts[i], replica, ol[i], cl_len) && hn == 2);
        uint8_t* mine = (uint8_t*)malloc(fl);
        uint32_t dw[16], sw[16];
        memcpy(dw, dig + 64 * i, 64);
        memcpy(sw, sig + 64 * i, 64);
        auto put = [mine](uint32_t pos, uint8_t b) { mine[pos] = b; };
        CHECK(pr_write_frame(put, view, first + i, dw, ops + off[i], ol[i], ts[i], cl, cl_len, replica, sw) == fl);
        CHECK(memcmp(mine, fr, fl) == 0);
        free(mine);
        ++canon;
      }
      // back through the general parser (its own copy of exactly the body)
      char* js = (char*)malloc(body ? body : 1);
      memcpy(js, fr + hn, body);
      char* arena = (char*)malloc(body + 16);
      pbft_wire_msg m;
      const bool parses = cl_len >= 1 && cl_len <= 63;  // (the parser refuses a client that does not fit its field)
      CHECK((pbft_wire_decode_json(js, body, &m, arena, body + 16) == 0) == parses);
      if (parses) {
        CHECK(m.kind == PBFT_MSG_PREPREPARE && m.view == view && m.seq == first + i && m.digest_ok && m.has_sig);
        CHECK(m.replica == replica && m.timestamp == ts[i] && m.operation_len == ol[i]);
        CHECK(memcmp(m.digest, dig + 64 * i, 64) == 0 && memcmp(m.sig, sig + 64 * i, 64) == 0);
        CHECK(ol[i] == 0 || memcmp(m.operation, ops + off[i], ol[i]) == 0);
        CHECK(strlen(m.client) == cl_len && memcmp(m.client, cl, cl_len) == 0);
      }
      // and through the canonical matcher
      pbft_pp_head h;
      CHECK(decode_preprepare((const uint8_t*)js, body, &h) == 0);
      CHECK((h.status == PBFT_PP_OK) == can);
      if (can) {
        CHECK(h.view == view && h.seq == first + i && h.timestamp == ts[i] && h.replica == replica);
        CHECK(h.op_len == ol[i] && (ol[i] == 0 || memcmp(js + h.op_off, ops + off[i], ol[i]) == 0));
        CHECK(memcmp(h.claimed, dig + 64 * i, 64) == 0 && memcmp(h.sig, sig + 64 * i, 64) == 0);
      }
      free(arena);
      free(js);
      ++frames;
    }
    free(st);
    free(foff);
    free(out);
    free(sig);
    free(dig);
    free(ops);
    free(clients);
  }
  // the wrap of first_seq + i
  {
    const uint64_t o2[2] = {0, 0};
    const uint32_t l2[2] = {0, 0};
    const uint64_t t2[2] = {1, 2};
    char c2[128] = "a";
    c2[64] = 'b';
    size_t need = 7;
    CHECK(pbft_wire_encode_preprepares(2, 1, ~0ull, nullptr, o2, l2, t2, c2, 0, nullptr, nullptr, nullptr, 0, &need,
                                       nullptr, nullptr) == PBFT_EINVAL);
    CHECK(pbft_wire_encode_preprepares(2, 1, ~0ull - 1, nullptr, o2, l2, t2, c2, 0, nullptr, nullptr, nullptr, 0, &need,
                                       nullptr, nullptr) == 0);
    CHECK(need == 2 * (2 + PR_BODY_MIN + 19));
  }
  printf("propose host run ok: %llu frames, %llu canonical\n", (unsigned long long)frames, (unsigned long long)canon);
  return 0;
}
