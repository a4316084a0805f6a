// Device helpers shared by the wire kernels that sign or hash one item per lane and write a tile's texts behind each
// other (egress.hip, propose.hip, reply.hip, accept.hip): the wave scan and shuffle, the span test and the aligned-dword
// reader, Blake2b-512 over a span, the client field and the envelope as words, and the head | body | tail writer of one
// tile.  Device only, every function inlined; the host + device text rules stay in the *_core.h headers, and the second
// half of RFC 8032 signing is sign_expanded (verify_core.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "digest_kernels.h"
#include "propose_core.h"

namespace pbft {

__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
  const uint32_t lo = __shfl((uint32_t)v, src, 64), hi = __shfl((uint32_t)(v >> 32), src, 64);
  return ((uint64_t)hi << 32) | lo;
}

// Does the span [off, off + len) lie inside [0, bytes)?  (Decided before any address is formed.)
__device__ __forceinline__ bool span_inside(uint64_t off, uint32_t len, uint64_t bytes) {
  return len <= bytes && off <= bytes - len;
}

// Bytes [o, o + 4) of the string m[0, len) as a little-endian word, zero past the end, through aligned dwords of which
// at least one byte belongs to the string: for a string inside [base, base + bytes) with base 4-byte aligned, every
// byte read lies in [base, round_up(bytes, 4)).
__device__ __forceinline__ uint32_t load32_span(const uint8_t* m, uint64_t len, uint64_t o) {
  if (o >= len) return 0u;
  const uintptr_t a = (uintptr_t)(m + o);
  const uint32_t* q = (const uint32_t*)(a & ~(uintptr_t)3);
  const uint32_t mis = (uint32_t)(a & 3);
  const uint32_t lo = q[0];
  const uint32_t hi = (mis && o + (4 - mis) < len) ? q[1] : 0u;
  uint32_t w = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * mis));
  const uint64_t rem = len - o;
  if (rem < 4) w &= (1u << (8 * (uint32_t)rem)) - 1u;
  return w;
}

// Blake2b-512 as 16 little-endian words, the string read where it lies (load32_span).  PREFIX = false: of m[0, len).
// PREFIX = true: of C | m[0, len), where the first eight message words of block 0 are cw (client_words) and the hashed
// length is PR_CLIENT_FIELD + len.
template <bool PREFIX>
__device__ __forceinline__ void blake2b512_span(uint32_t out[16], const uint64_t cw[8], const uint8_t* m, uint64_t len) {
  uint64_t h[8] = {0x6a09e667f3bcc908ULL ^ 0x01010040ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL,
                   0xa54ff53a5f1d36f1ULL, 0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL,
                   0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
  constexpr uint64_t pre = PREFIX ? PR_CLIENT_FIELD : 0;
  const uint64_t total = pre + len;
  const uint64_t nblocks = (!PREFIX && len == 0) ? 1 : (total + 127) / 128;  // (the empty string: one block)
  for (uint64_t b = 0; b < nblocks; ++b) {
    uint64_t mw[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (PREFIX && b == 0 && j < 8) {
        mw[j] = cw[j];
      } else {
        const uint64_t o = 128 * b + 8 * j - pre;
        mw[j] = ((uint64_t)load32_span(m, len, o + 4) << 32) | load32_span(m, len, o);
      }
    }
    const bool last = b == nblocks - 1;
    blake2b_compress(h, mw, last ? total : 128 * (b + 1), last);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    out[2 * i] = (uint32_t)h[i];
    out[2 * i + 1] = (uint32_t)(h[i] >> 32);
  }
}

// C as eight little-endian words: the client field up to its first NUL, zeros behind it.
__device__ __forceinline__ void client_words(uint64_t cw[8], const uint8_t* field) {
  bool open = true;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    uint64_t w = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint32_t b = field[8 * j + k];
      open = open && b != 0;
      w |= (uint64_t)(open ? b : 0u) << (8 * k);
    }
    cw[j] = w;
  }
}

// The wave tests the spans of the lanes that are candidates against the texts' alphabet (pr_alphabet), span after span,
// 64 bytes per step with one ballot per span; a lane learns about its own span.  cand implies that the span lies
// inside text.
__device__ __forceinline__ bool wave_span_alphabet(const uint8_t* text, bool cand, uint64_t off, uint32_t len, int lane) {
  bool mine = true;
  for (int r = 0; r < 64; ++r) {
    if (!__shfl((int)cand, r, 64)) continue;  // (wave-uniform)
    const uint64_t o = shfl64(off, r);
    const uint32_t l = __shfl(len, r, 64);
    bool bad = false;
    for (uint32_t k = lane; k < l; k += 64) bad = bad || !pr_alphabet(text[o + k]);
    const bool any = __ballot(bad) != 0;
    if (lane == r) mine = !any;
  }
  return mine;
}

struct lds_sink {
  uint8_t* p;
  __device__ __forceinline__ void operator()(uint32_t pos, uint8_t b) const { p[pos] = b; }
};

// An envelope's LDS row in dwords: 85 bytes, zero-padded; odd, so that the 64 lanes' bytewise writes at one row position
// fall into 64 different banks
static constexpr uint32_t ENV_ROW_DWORDS = 25;
static_assert(4 * ENV_ROW_DWORDS >= 96 && ENV_ROW_DWORDS % 2 == 1, "");

// "PBFT" | kind | view | n | D into the row e, zeros behind it: the hashes read it through aligned dwords
__device__ __forceinline__ void envelope_row(uint8_t* e, uint32_t kind, uint64_t view, uint64_t n, const uint32_t dg[16]) {
  e[0] = 'P', e[1] = 'B', e[2] = 'F', e[3] = 'T', e[4] = (uint8_t)kind;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    e[5 + j] = (uint8_t)(view >> (8 * j));
    e[13 + j] = (uint8_t)(n >> (8 * j));
  }
#pragma unroll
  for (int j = 0; j < 64; ++j) e[21 + j] = (uint8_t)(dg[j >> 2] >> (8 * (j & 3)));
#pragma unroll
  for (int j = EG_ENV_BYTES; j < 4 * (int)ENV_ROW_DWORDS; ++j) e[j] = 0;
}

// The wave writes the tile's texts one after the other.  Lane r holds text r's head, body and tail lengths (hl = 0: no
// text), its body's offset in src_base and its offset local behind out + base; the head and tail lie in r's rows of
// s_head and s_tail.  Byte k of text r comes from the head row, from the body in global memory or from the tail row;
// lane l moves the W bytes of store l, l + 64, ...  W = 1: bytewise; W = 4 / 16: the output's aligned dwords / 16-byte
// granules with one store each, the text's unaligned ends bytewise.  Nothing outside [dst, dst + hl + body_len + tl) is
// written, so the caller's test against the output's capacity (whole texts only) is the bound.
template <int W, uint32_t HEAD_DWORDS, uint32_t TAIL_DWORDS>
__device__ __forceinline__ void tile_copy(int lane, uint32_t hl, uint32_t body_len, uint32_t tl, uint64_t off,
                                          uint32_t local, uint64_t base, const uint32_t (&s_head)[64][HEAD_DWORDS],
                                          const uint32_t (&s_tail)[64][TAIL_DWORDS], const uint8_t* src_base,
                                          uint8_t* out) {
  for (int r = 0; r < 64; ++r) {
    const uint32_t h = __shfl(hl, r, 64);
    if (h == 0) continue;  // (wave-uniform)
    const uint32_t l = __shfl(body_len, r, 64), t = __shfl(tl, r, 64);
    const uint64_t o = shfl64(off, r);
    const uint32_t len = h + l + t;
    uint8_t* dst = out + base + __shfl(local, r, 64);
    const uint8_t* hr = (const uint8_t*)s_head[r];
    const uint8_t* tr = (const uint8_t*)s_tail[r];
    const uint8_t* src = src_base + o;
    auto byte = [&](uint32_t k) -> uint32_t { return k < h ? hr[k] : (k < h + l ? src[k - h] : tr[k - h - l]); };
    if constexpr (W == 1) {
      for (uint32_t k = lane; k < len; k += 64) dst[k] = (uint8_t)byte(k);
    } else {
      uint32_t head = (uint32_t)((W - ((uintptr_t)dst & (W - 1))) & (W - 1));
      if (head > len) head = len;
      const uint32_t words = (len - head) / W;
      for (uint32_t k = lane; k < head; k += 64) dst[k] = (uint8_t)byte(k);
      for (uint32_t wd = lane; wd < words; wd += 64) {
        const uint32_t k0 = head + W * wd;
        uint32_t v[W / 4];
#pragma unroll
        for (int j = 0; j < W / 4; ++j)
          v[j] = byte(k0 + 4 * j) | byte(k0 + 4 * j + 1) << 8 | byte(k0 + 4 * j + 2) << 16 | byte(k0 + 4 * j + 3) << 24;
        if constexpr (W == 4) *(uint32_t*)(dst + k0) = v[0];
        else *(uint4*)(dst + k0) = make_uint4(v[0], v[1], v[2], v[3]);
      }
      for (uint32_t k = head + W * words + lane; k < len; k += 64) dst[k] = (uint8_t)byte(k);
    }
  }
}

}  // namespace pbft
