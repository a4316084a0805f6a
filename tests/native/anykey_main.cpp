// TEST INFRASTRUCTURE: anykey_core.h's host build as a stand-alone program (tests/test_anykey.py compiles it with
// AddressSanitizer + UBSan and runs it directly).  The base-point table is a small plan's (14 x 7 + 26 x 6 bits, the
// balanced shape of the GPU's plan incl. its undecoded top window), built here by doubling and repeated addition.
//
//   anykey_main IN OUT
// IN: records, each a header of four little-endian u32 (mode, n, msg_len, msg_stride) and then
//   mode 0 (verify): R[n][32] S[n][32] A[n][32] msg[n][msg_stride]   -> OUT: n bytes, 1 = accepted
//   mode 1 (point):  s[n][32] k[n][32] A[n][32]                      -> OUT: enc[n][32] then key_ok[n]
// until the end of the file.  Exit status 0 and "anykey host run ok: <records> records, <items> items" on success.
#include "../../pbft_amd/csrc/anykey_core.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace pbft;

using PLAN_H = plan<40, 6, 14>;

static void words_from_bytes(uint32_t w[8], const uint8_t* b) {
  for (int i = 0; i < 8; ++i)
    w[i] = b[4 * i] | (b[4 * i + 1] << 8) | (b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
}
static void bytes_from_words(uint8_t* b, const uint32_t w[8]) {
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 4; ++j) b[4 * i + j] = (uint8_t)(w[i] >> (8 * j));
}

// verify_lane's R check (verify_core.h): R' equals the point r_enc decompresses to, which is not of small order
static bool matches_r(const ge& P, const uint32_t r_enc[8]) {
  uint32_t enc[8], yw[8], ry[8];
  ge_compress_words(enc, P);
  for (int i = 0; i < 8; ++i) yw[i] = enc[i];
  yw[7] &= 0x7fffffffu;
  canon_y(ry, r_enc);
  bool eq = (enc[7] >> 31) == (r_enc[7] >> 31);
  for (int i = 0; i < 8; ++i) eq = eq && yw[i] == ry[i];
  return eq && !y_is_small_order(yw);
}

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: anykey_main IN OUT\n"); return 2; }
  std::vector<uint32_t> tabB(PLAN_H::TABLE_WORDS);
  {
    static const uint8_t Benc[32] = {0x58, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66,
                                     0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66,
                                     0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66};
    uint32_t e[8];
    ge B;
    words_from_bytes(e, Benc);
    if (!ge_decompress(B, e)) return 3;
    for (int pos = 0; pos < PLAN_H::P; ++pos) {
      // entries j * 2^bitoff(pos) * B: the position's base by doublings, then repeated addition
      niels n;
      niels_identity(n);
      store_niels(tabB.data() + (size_t)PLAN_H::offset(pos) * 32, n);
      ge base;
      {
        ge Q = B;
        for (int i = 0; i < PLAN_H::bitoff(pos); ++i) ge_dbl(Q, Q);
        base = Q;
      }
      ge acc = base;
      for (uint32_t j = 1; j < PLAN_H::entries(pos); ++j) {
        ge_to_niels(n, acc);
        store_niels(tabB.data() + ((size_t)PLAN_H::offset(pos) + j) * 32, n);
        ge t;
        ge_add(t, acc, base);
        acc = t;
      }
    }
  }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
  unsigned records = 0;
  unsigned long items = 0;
  for (;;) {
    uint32_t hd[4];
    const size_t got = fread(hd, 1, sizeof hd, in);
    if (got == 0) break;
    if (got != sizeof hd) { fprintf(stderr, "short header\n"); return 4; }
    const uint32_t mode = hd[0], n = hd[1], msg_len = hd[2], msg_stride = hd[3];
    if (mode > 1 || n > (1u << 20) || msg_stride < msg_len || msg_stride > (1u << 16)) { fprintf(stderr, "bad header\n"); return 4; }
    std::vector<uint8_t> a((size_t)32 * n), b((size_t)32 * n), c((size_t)32 * n);
    // (+ 16: the hash reads the message in aligned pieces, as the kernels' callers provide for)
    std::vector<uint8_t> msg(mode == 0 ? (size_t)msg_stride * n + 16 : 0);
    if (!read_exact(in, a.data(), a.size()) || !read_exact(in, b.data(), b.size()) || !read_exact(in, c.data(), c.size()) ||
        (mode == 0 && !read_exact(in, msg.data(), (size_t)msg_stride * n))) {
      fprintf(stderr, "short record\n");
      return 4;
    }
    std::vector<uint8_t> res(mode == 0 ? (size_t)n : (size_t)33 * n);
    for (uint32_t i = 0; i < n; ++i) {
      uint32_t x[8], y[8], key[8];
      words_from_bytes(x, a.data() + 32 * (size_t)i);
      words_from_bytes(y, b.data() + 32 * (size_t)i);
      words_from_bytes(key, c.data() + 32 * (size_t)i);
      ge P;
      if (mode == 0) {
        const uint8_t* m = msg.data() + (size_t)msg_stride * i;
        const bool flag = msg_len == 85 ? anykey_lane<PLAN_H, 85>(P, x, y, key, m, 85, tabB.data())
                                        : anykey_lane<PLAN_H, -1>(P, x, y, key, m, (int)msg_len, tabB.data());
        res[i] = flag && matches_r(P, x);
      } else {
        bool key_ok;
        anykey_sum<PLAN_H>(P, x, y, key, tabB.data(), key_ok);
        uint32_t enc[8];
        ge_compress_words(enc, P);
        bytes_from_words(res.data() + 32 * (size_t)i, enc);
        res[(size_t)32 * n + i] = key_ok;
      }
    }
    if (fwrite(res.data(), 1, res.size(), out) != res.size()) return 5;
    ++records;
    items += n;
  }
  fclose(in);
  if (fclose(out) != 0) return 5;
  printf("anykey host run ok: %u records, %lu items\n", records, items);
  return 0;
}
