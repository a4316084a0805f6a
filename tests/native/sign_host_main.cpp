// The pure-host half of the blocking signing forms (pbft_amd/csrc/sign_host.h) as a stand-alone program, for
// AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_sign_host.py), linked with the host encoders
// (pbft_amd/csrc/host/wire.cpp):
//   * sign_layout against the offsets pbft_sign_replies and pbft_sign_votes_frames used to write out by hand: regions in
//     order, 256-aligned, large enough, not overlapping, the total the last region's end;
//   * sign_spans_inside at its edges;
//   * sign_count and sign_merge over mixes of device-written and general items: the "device" bytes are the OK items of
//     pbft_wire_encode_preprepares / pbft_wire_encode_replies over the whole batch, packed into a heap buffer of exactly
//     their size, the callback is the one-item call of the entry points, the output a heap buffer of exactly the
//     stream's length plus guard bytes -- so a read or a write of one byte outside is a sanitizer report -- and the
//     merged stream must equal the whole-batch encoding; a callback that fails or reports another length is an error.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pbft_wire.h"
#include "../../pbft_amd/csrc/sign_host.h"

using namespace pbft;

#define CHECK(x)                                                              \
  do {                                                                        \
    if (!(x)) {                                                               \
      fprintf(stderr, "sign_host_main: %s failed (line %d)\n", #x, __LINE__); \
      return 1;                                                               \
    }                                                                         \
  } while (0)

// wire.cpp's vote decoder refers to pbft_envelope (host/replica.cpp, which is not linked here); never called
extern "C" void pbft_envelope(uint8_t*, uint8_t, uint64_t, uint64_t, const uint8_t*) { abort(); }

static size_t up(size_t b) { return (b + 255) & ~(size_t)255; }

// ---- the layout ----
static int check_layout(uint64_t N, size_t B, size_t D) {
  const sign_layout L(N, B, D);
  // the closed form of pbft_sign_replies
  const size_t oOff = up(B + 16), oLen = oOff + up(8 * (size_t)N), oTs = oLen + up(4 * (size_t)N),
               oCl = oTs + up(8 * (size_t)N), oF = oCl + up(64 * (size_t)N), oD = oF + up(8 * (size_t)(N + 1)),
               oS = oD + up(64 * (size_t)N), oSt = oS + up(64 * (size_t)N), oO = oSt + up(N);
  const size_t total = oO + up(D);
  CHECK(L.off == oOff && L.len == oLen && L.ts == oTs && L.cl == oCl && L.out_off == oF && L.dig == oD && L.sig == oS &&
        L.st == oSt && L.out == oO && L.total == total);
  const size_t start[11] = {0, L.off, L.len, L.ts, L.cl, L.out_off, L.dig, L.sig, L.st, L.out, L.total};
  const size_t need[10] = {B + 16, 8 * (size_t)N, 4 * (size_t)N, 8 * (size_t)N, 64 * (size_t)N, 8 * (size_t)(N + 1),
                           64 * (size_t)N, 64 * (size_t)N, (size_t)N, D};
  for (int r = 0; r < 10; ++r) {
    CHECK(start[r] % 256 == 0);
    CHECK(start[r + 1] >= start[r]);                // in order
    CHECK(start[r + 1] - start[r] >= need[r]);      // large enough, and the next begins behind it: no overlap
    CHECK(start[r + 1] - start[r] < need[r] + 256);  // and no more than the rounding
  }
  CHECK(L.total % 256 == 0 && L.total == L.out + up(D));
  return 0;
}

static int check_votes_layout(uint64_t N, uint32_t stride, size_t need) {
  const sign_layout L = sign_votes_layout(stride, N, need);
  // the closed form of pbft_sign_votes_frames
  const size_t env_bytes = (size_t)stride * (N - 1) + EG_ENV_BYTES;
  const size_t offF = up(env_bytes), offS = offF + up(8 * (size_t)(N + 1)), offO = offS + up(64 * (size_t)N);
  CHECK(sign_votes_env_bytes(stride, N) == env_bytes);
  CHECK(L.out_off == offF && L.sig == offS && L.out == offO && L.total == offO + up(need));
  CHECK(L.off == offF && L.len == offF && L.ts == offF && L.cl == offF);  // the unused regions are empty
  CHECK(L.dig == L.sig && L.st == L.out);
  CHECK(offF >= env_bytes && offS - offF >= 8 * (N + 1) && offO - offS >= 64 * N && L.total - offO >= need);
  CHECK(offF % 256 == 0 && offS % 256 == 0 && offO % 256 == 0 && L.total % 256 == 0);
  return 0;
}

// ---- the span check ----
static bool inside(uint64_t off, uint32_t len, uint64_t bytes) { return sign_spans_inside(&off, &len, 1, bytes); }

static int check_spans() {
  CHECK(inside(0, 1000, 1000));               // len == bytes at off 0
  CHECK(inside(1000, 0, 1000));               // off == bytes with len 0
  CHECK(!inside(1001, 0, 1000));
  CHECK(inside(999, 1, 1000) && !inside(999, 2, 1000) && !inside(1, 1000, 1000));  // one past the end
  CHECK(!inside(1ull << 63, 0, 1000) && !inside(1ull << 63, 1, 1000));
  CHECK(!inside(~0ull, 1, 1000) && !inside(~0ull - 3, 4, 1000));  // off + len would wrap
  CHECK(!inside(0, 0xffffffffu, 1000));
  CHECK(inside(0, 0xffffffffu, 0xffffffffull) && !inside(1, 0xffffffffu, 0xffffffffull));
  CHECK(inside(1ull << 63, 0xffffffffu, ~0ull) && !inside(~0ull, 1, ~0ull) && inside(~0ull, 0, ~0ull));
  CHECK(inside(0, 0, 0) && !inside(1, 0, 0) && !inside(0, 1, 0));
  CHECK(sign_spans_inside(nullptr, nullptr, 0, 0));
  const uint64_t off[3] = {0, 10, 20};
  const uint32_t len[3] = {10, 10, 10}, bad[3] = {10, 10, 11};
  CHECK(sign_spans_inside(off, len, 3, 30) && !sign_spans_inside(off, len, 3, 29) && !sign_spans_inside(off, bad, 3, 30));
  return 0;
}

// ---- the merge ----
// N items, item i general where mix[i] is 'g': a quote is outside the canonical alphabet of both encoders.
struct Batch {
  uint64_t N;
  std::vector<uint8_t> data;
  std::vector<uint64_t> off, ts;
  std::vector<uint32_t> len;
  std::vector<char> clients;
  std::vector<uint8_t> dig, sig;
  explicit Batch(const std::string& mix) : N(mix.size()) {
    for (uint64_t i = 0; i < N; ++i) {
      std::string item = "item-" + std::to_string(i) + std::string(7 * i % 40, 'x');
      if (mix[i] == 'g') item += " \"quoted\"\n";
      off.push_back(data.size());
      len.push_back((uint32_t)item.size());
      data.insert(data.end(), item.begin(), item.end());
      ts.push_back(i % 3 == 0 ? ~0ull - i : 10 * i + 9);
      char cl[64] = {0};
      snprintf(cl, sizeof cl, "127.0.0.1:%u", 8080 + (unsigned)i);
      clients.insert(clients.end(), cl, cl + 64);
    }
    dig.resize(64 * N);
    sig.resize(64 * N);
    for (size_t k = 0; k < 64 * N; ++k) {
      dig[k] = (uint8_t)(k * 37 + 1);
      sig[k] = (uint8_t)(k * 101 + 7);
    }
  }
};

static const uint32_t REPLICA = 2;
static const uint64_t VIEW = 9999999999999999999ull, FIRST = 0xffffffffull - 2;
static const size_t GUARD = 64;
static char PEER_ID[52];

// form 0: PrePrepare frames; form 1: reply texts
static int whole(int form, const Batch& b, uint8_t* out, size_t cap, size_t* len, uint64_t* off, uint8_t* st) {
  return form == 0 ? pbft_wire_encode_preprepares(b.N, VIEW, FIRST, b.data.data(), b.off.data(), b.len.data(),
                                                  b.ts.data(), b.clients.data(), REPLICA, b.dig.data(), b.sig.data(), out,
                                                  cap, len, off, st)
                   : pbft_wire_encode_replies(b.N, VIEW, b.ts.data(), b.data.data(), b.off.data(), b.len.data(), REPLICA,
                                              PEER_ID, b.sig.data(), out, cap, len, off, st);
}

static int check_merge(int form, const std::string& mix) {
  const Batch b(mix);
  const uint64_t N = b.N;
  const uint8_t OK = form == 0 ? PBFT_PROPOSE_OK : PBFT_REPLY_OK;
  std::vector<uint64_t> h_off(N + 1);
  std::vector<uint8_t> h_st(N);
  size_t need = 0;
  CHECK(whole(form, b, nullptr, 0, &need, h_off.data(), h_st.data()) == 0);  // the dry run of the entry points
  CHECK(need > 0 && h_off[0] == 0 && h_off[N] == need);
  std::vector<uint8_t> want(need);
  size_t got_len = 0;
  CHECK(whole(form, b, want.data(), need, &got_len, nullptr, nullptr) == 0 && got_len == need);
  size_t dev_bytes = 0;
  uint64_t n_general = 0;
  for (uint64_t i = 0; i < N; ++i) {
    CHECK((h_st[i] != OK) == (mix[i] == 'g'));  // the mix is the one asked for
    if (h_st[i] == OK) dev_bytes += (size_t)(h_off[i + 1] - h_off[i]);
    else ++n_general;
  }
  const sign_split s = sign_count(h_off.data(), h_st.data(), N, OK);
  CHECK(s.n_general == n_general && s.dev_bytes == dev_bytes);
  // what the device writes: the OK items back to back, in a buffer of exactly that size (none: no buffer at all)
  uint8_t* dev = dev_bytes ? (uint8_t*)malloc(dev_bytes) : nullptr;
  size_t at = 0;
  for (uint64_t i = 0; i < N; ++i)
    if (h_st[i] == OK) {
      memcpy(dev + at, want.data() + h_off[i], (size_t)(h_off[i + 1] - h_off[i]));
      at += (size_t)(h_off[i + 1] - h_off[i]);
    }
  CHECK(at == dev_bytes);
  uint8_t* out = (uint8_t*)malloc(need + GUARD);
  const uint64_t off1 = 0;
  uint64_t calls = 0;
  int fail_at = -1, wrong_len_at = -1;
  auto general = [&](uint64_t i, uint8_t* to, size_t fl, size_t* got) {
    ++calls;
    if ((int)i == fail_at) return -1;
    const int rc =
        form == 0 ? pbft_wire_encode_preprepares(1, VIEW, FIRST + i, b.data.data() + b.off[i], &off1, b.len.data() + i,
                                                 b.ts.data() + i, b.clients.data() + 64 * i, REPLICA,
                                                 b.dig.data() + 64 * i, b.sig.data() + 64 * i, to, fl, got, nullptr,
                                                 nullptr)
                  : pbft_wire_encode_replies(1, VIEW, b.ts.data() + i, b.data.data() + b.off[i], &off1, b.len.data() + i,
                                             REPLICA, PEER_ID, b.sig.data() + 64 * i, to, fl, got, nullptr, nullptr);
    if ((int)i == wrong_len_at) --*got;
    return rc;
  };
  memset(out, 0xA5, need + GUARD);
  CHECK(sign_merge(N, h_off.data(), h_st.data(), OK, dev, out, general));
  CHECK(calls == n_general);
  CHECK(memcmp(out, want.data(), need) == 0);
  for (size_t k = 0; k < GUARD; ++k) CHECK(out[need + k] == 0xA5);
  if (n_general) {  // the last general item fails, then reports one byte less
    int last = -1;
    for (uint64_t i = 0; i < N; ++i)
      if (mix[i] == 'g') last = (int)i;
    fail_at = last;
    CHECK(!sign_merge(N, h_off.data(), h_st.data(), OK, dev, out, general));
    fail_at = -1;
    wrong_len_at = last;
    CHECK(!sign_merge(N, h_off.data(), h_st.data(), OK, dev, out, general));
    for (size_t k = 0; k < GUARD; ++k) CHECK(out[need + k] == 0xA5);
  }
  free(out);
  free(dev);
  return 0;
}

int main() {
  int layouts = 0, merges = 0;
  for (uint64_t N : {1, 2, 63, 64, 65})
    for (size_t B : {0, 1, 255, 256, 257})
      for (size_t D : {0, 1, 255, 256, 257, 100000}) {
        if (check_layout(N, B, D)) return 1;
        ++layouts;
      }
  for (uint64_t N : {1, 2, 63, 64, 65, 193})
    for (uint32_t stride : {85, 96, 256})
      for (size_t need : {0, 338, 381 * 193}) {
        if (check_votes_layout(N, stride, need)) return 1;
        ++layouts;
      }
  if (check_spans()) return 1;
  memset(PEER_ID, '1', sizeof PEER_ID);  // (52 base58 characters; the encoder copies them)
  std::string alternating, alternating2;
  for (int i = 0; i < 65; ++i) {
    alternating += i & 1 ? 'g' : 'd';
    alternating2 += i & 1 ? 'd' : 'g';
  }
  const std::string mixes[] = {std::string(7, 'd'),         std::string(7, 'g'), "g" + std::string(9, 'd'),
                               std::string(9, 'd') + "g",   alternating,         alternating2,
                               "d",                         "g",                 "gdddddddg"};
  for (int form = 0; form < 2; ++form)
    for (const std::string& mix : mixes) {
      if (check_merge(form, mix)) return 1;
      ++merges;
    }
  printf("sign host run ok: %d layouts, %d merges\n", layouts, merges);
  return 0;
}
