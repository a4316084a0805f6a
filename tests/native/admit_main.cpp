// TEST INFRASTRUCTURE: the host build of the replica's admission rule (pbft_amd/csrc/admit_core.h, the code each GPU
// lane runs in admit.hip: classify, the two key planes, resolve, the residue's prefix sum and emit) under
// AddressSanitizer + UndefinedBehaviorSanitizer.  Built and run by tests/test_admit.py, host only: it reads cases
// (parameters and a pbft_frame_head array each) from a file, writes every output of pbft_admit_device for them to
// another, and the test compares those with pbft_amd.admit_reference.  Here the loops over lanes are plain loops; the
// planes are heap vectors of exactly admit_plane_bits bits (rounded up to a 32-bit word), so a key outside them is a
// heap overflow.  Every case runs twice, rows marked in ascending and in descending order: the outputs must not
// depend on the order in which the plane updates land.
//
// Input:  u64 n_cases, then per case u64 {N, n_total, view, h, log_window, n_keys, residue_cap}, N heads of 24
//         bytes, N u64 off, N u32 len.
// Output: per case cls [N] u8, counts [8] u32, clean [ceil(N / 64)] u64, res [residue_cap] 16 bytes, n_res [2] u32,
//         keep [N] u8 (1: the record keeps its key index).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/pbft_wire.h"
#include "../../pbft_amd/csrc/admit_core.h"

using namespace pbft;

#define CHECK(c)                                                             \
  do {                                                                       \
    if (!(c)) {                                                              \
      fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); \
      exit(1);                                                               \
    }                                                                        \
  } while (0)

static_assert(sizeof(admit_head) == sizeof(pbft_frame_head), "admit_head is pbft_frame_head");
static_assert(PBFT_ADMIT_PAD == ADMIT_PAD && PBFT_ADMIT_HOST == ADMIT_HOST && PBFT_ADMIT_CLASSES == ADMIT_CLASSES, "");

struct Out {
  std::vector<uint8_t> cls, keep;
  std::vector<uint32_t> counts;
  std::vector<uint64_t> clean;
  std::vector<pbft_admit_residue> res;
  uint32_t n_res[2];
};

// What launch_admit enqueues, lane by lane; `descending`: the order of the mark lanes.
static Out host_admit(const std::vector<admit_head>& heads, const std::vector<uint64_t>& off,
                      const std::vector<uint32_t>& len, uint64_t n_total, uint64_t view, uint64_t h, uint64_t W,
                      uint32_t n_keys, uint32_t residue_cap, bool descending) {
  const uint64_t N = heads.size(), n_valid = n_total < N ? n_total : N, words = (N + 63) / 64;
  const uint64_t bits = admit_plane_bits(W, n_keys);
  CHECK(bits != 0);
  std::vector<uint32_t> seen((bits + 31) / 32, 0), twice((bits + 31) / 32, 0);  // zero kernel
  Out o;
  o.cls.assign(N, 0xEE);
  o.keep.assign(N, 1);
  o.counts.assign(ADMIT_CLASSES, 0);
  o.clean.assign(words, 0);
  o.res.assign(residue_cap, pbft_admit_residue{~0ull, ~0u, ~0u});
  for (uint64_t j = 0; j < N; ++j) {  // mark
    const uint64_t i = descending ? N - 1 - j : j;
    const uint32_t c = admit_classify(heads[i], i, n_valid, view, h, W, n_keys);
    o.cls[i] = (uint8_t)c;
    if (c == ADMIT_CLEAN) {
      const uint64_t k = admit_key(heads[i], h, n_keys);
      CHECK(k < bits);
      const uint32_t bit = 1u << (k & 31);
      const uint32_t old = seen.at(k >> 5);
      seen.at(k >> 5) = old | bit;
      if (old & bit) twice.at(k >> 5) |= bit;
    }
  }
  std::vector<uint64_t> flags(words, 0);
  for (uint64_t i = 0; i < N; ++i) {  // resolve
    uint32_t c = o.cls[i];
    if (c == ADMIT_CLEAN) {
      const uint64_t k = admit_key(heads[i], h, n_keys);
      if ((twice.at(k >> 5) >> (k & 31)) & 1) o.cls[i] = (uint8_t)(c = ADMIT_CONTESTED);
    }
    if (c != ADMIT_CLEAN) o.keep[i] = 0;
    CHECK(c < ADMIT_CLASSES);
    ++o.counts[c];
    if (c == ADMIT_CLEAN) o.clean[i >> 6] |= (uint64_t)1 << (i & 63);
    if (admit_is_residue(c)) flags[i >> 6] |= (uint64_t)1 << (i & 63);
  }
  std::vector<uint32_t> prefix(words, 0);  // scan
  uint32_t carry = 0;
  for (uint64_t w = 0; w < words; ++w) {
    prefix[w] = carry;
    carry += (uint32_t)__builtin_popcountll(flags[w]);
  }
  o.n_res[0] = carry;
  o.n_res[1] = carry > residue_cap ? carry - residue_cap : 0;
  for (uint64_t j = carry < residue_cap ? carry : residue_cap; j < residue_cap; ++j)  // emit
    o.res.at(j) = pbft_admit_residue{0, 0, 0};
  for (uint64_t i = 0; i < N; ++i) {
    const uint64_t w = flags[i >> 6];
    if (!((w >> (i & 63)) & 1)) continue;
    const uint32_t at = prefix[i >> 6] + (uint32_t)__builtin_popcountll(w & (((uint64_t)1 << (i & 63)) - 1));
    if (at >= residue_cap) continue;
    o.res.at(at) = pbft_admit_residue{off[i], (uint32_t)i, len[i]};
  }
  return o;
}

template <class T>
static void get(FILE* f, T* p, size_t n) {
  if (n) CHECK(fread(p, sizeof(T), n, f) == n);
}
template <class T>
static void put(FILE* f, const T* p, size_t n) {
  if (n) CHECK(fwrite(p, sizeof(T), n, f) == n);
}

int main(int argc, char** argv) {
  CHECK(argc == 3);
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  CHECK(in && out);
  uint64_t n_cases = 0, rows = 0;
  get(in, &n_cases, 1);
  for (uint64_t c = 0; c < n_cases; ++c) {
    uint64_t p[7];
    get(in, p, 7);
    const uint64_t N = p[0];
    CHECK(N <= (1u << 24) && p[5] >= 1 && p[5] <= 65535 && p[6] <= (1u << 24));
    std::vector<admit_head> heads(N);
    std::vector<uint64_t> off(N);
    std::vector<uint32_t> len(N);
    get(in, heads.data(), N);
    get(in, off.data(), N);
    get(in, len.data(), N);
    const Out a = host_admit(heads, off, len, p[1], p[2], p[3], p[4], (uint32_t)p[5], (uint32_t)p[6], false);
    const Out b = host_admit(heads, off, len, p[1], p[2], p[3], p[4], (uint32_t)p[5], (uint32_t)p[6], true);
    CHECK(a.cls == b.cls && a.keep == b.keep && a.counts == b.counts && a.clean == b.clean);
    CHECK(a.n_res[0] == b.n_res[0] && a.n_res[1] == b.n_res[1]);
    CHECK(a.res.size() == b.res.size() &&
          (a.res.empty() || memcmp(a.res.data(), b.res.data(), a.res.size() * sizeof(pbft_admit_residue)) == 0));
    put(out, a.cls.data(), N);
    put(out, a.counts.data(), a.counts.size());
    put(out, a.clean.data(), a.clean.size());
    put(out, a.res.data(), a.res.size());
    put(out, a.n_res, 2);
    put(out, a.keep.data(), N);
    rows += N;
  }
  fclose(in);
  CHECK(fclose(out) == 0);
  printf("admit host run ok: %llu cases, %llu rows\n", (unsigned long long)n_cases, (unsigned long long)rows);
  return 0;
}
