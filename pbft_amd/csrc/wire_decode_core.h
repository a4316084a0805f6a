// Decoder of the canonical signed-vote frame, shared by the host and the device (wire_decode.hip):
//   {"Prepare":{"view":V,"sequence_number":N,"digest":"<128 hex>","replica":R,"signature":"<128 hex>"}}
// (or "Commit"), the one form serde_json and pbft_wire_encode_json write.  The accept rule is byte for byte that of
// fast_vote (host/wire.cpp): decimal u64 without leading zero or overflow, lowercase hex, replica <= 65535, nothing
// after "}}".  Whatever is not that form is PBFT_WIRE_EDEFER: the general parser decides, with serde's rules.
//
// The frame is read through an accessor of aligned dwords, `uint32_t Rd::dword(uint32_t i) const`,
// i < FRAME_ROW_DWORDS: dword i holds bytes [4 i, 4 i + 4) of a row in which the frame occupies bytes [b0, b0 + n),
// b0 < 4.  The host reads memory, the kernel its wave's LDS rows.  Bytes of the row outside the frame may hold
// anything: every bound is checked before the bytes behind it are looked at, so no result depends on them.
#pragma once
#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__CUDACC__)
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

namespace pbft {

constexpr uint32_t WIRE_ST_OK = 0, WIRE_ST_ESIGNER = 5, WIRE_ST_EDEFER = 6;  // PBFT_WIRE_* of include/pbft_wire.h
constexpr uint32_t FRAME_MIN = 336;  // {"Commit":...} with three one-digit numbers
constexpr uint32_t FRAME_MAX = 379;  // {"Prepare":...} with two 20-digit numbers and a 5-digit replica
// Row of one frame: 3 + 379 bytes round up to 96 dwords.  97 is odd: lanes that read the same dword of their own rows
// (the canonical case: equal decimal widths) fall on 32 distinct LDS banks per half wave, where a stride of 96 dwords
// would put them all on one.
constexpr uint32_t FRAME_ROW_DWORDS = 97;
constexpr uint32_t FRAME_NO_PEER = 0xFFFFFFFFu;
constexpr uint32_t FRAME_NO_KEY = 0xFFFFu;  // key index of a record that is not PBFT_WIRE_OK: >= any key count

struct frame_fields {
  uint64_t view, seq;
  uint32_t key_idx, kind, status;
};

template <class Rd>
struct frame_cursor {
  const Rd& rd;
  // next byte and end of the frame, as byte positions in the row (e <= 382 for a vote's row; any row works whose
  // accessor serves the dword behind the one that holds byte e - 1: wire_pp_core.h's rows are longer)
  uint32_t p, e;

  // the 4 bytes at row position at (at < e), little endian; the upper ones may lie past the frame
  __host__ __device__ uint32_t word4(uint32_t at) const {
    const uint32_t i = at >> 2, s = (at & 3) * 8;
    const uint64_t w = ((uint64_t)rd.dword(i + 1) << 32) | rd.dword(i);
    return (uint32_t)(w >> s);
  }
  __host__ __device__ uint32_t byte(uint32_t at) const { return (rd.dword(at >> 2) >> ((at & 3) * 8)) & 0xFFu; }

  // the K1 - 1 characters of L
  template <unsigned K1>
  __host__ __device__ bool lit(const char (&L)[K1]) {
    constexpr uint32_t k = K1 - 1;
    if (p + k > e) return false;
    uint32_t bad = 0;
#pragma unroll
    for (uint32_t j = 0; j < k; j += 4) {
      uint32_t c = 0, m = 0;
#pragma unroll
      for (uint32_t b = 0; b < 4; ++b)
        if (j + b < k) {
          c |= (uint32_t)(uint8_t)L[j + b] << (8 * b);
          m |= 0xFFu << (8 * b);
        }
      bad |= (word4(p + j) ^ c) & m;
    }
    if (bad) return false;
    p += k;
    return true;
  }

  // serde's u64: digits, no leading zero, no overflow
  __host__ __device__ bool num(uint64_t* v) {
    if (p >= e) return false;
    const uint32_t c0 = byte(p) - '0';
    if (c0 > 9) return false;
    if (c0 == 0 && p + 1 < e && byte(p + 1) - '0' <= 9u) return false;
    constexpr uint64_t TOP = 1844674407370955161ull;  // (2^64 - 1) / 10; the last digit may then be at most 5
    uint64_t x = 0;
    while (p < e) {  // four characters per read
      uint32_t w = word4(p);
      const uint32_t stop = p + 4 < e ? p + 4 : e;
      for (; p < stop; ++p, w >>= 8) {
        const uint32_t d = (w & 0xFFu) - '0';
        if (d > 9) {
          *v = x;
          return true;
        }
        if (x > TOP || (x == TOP && d > 5)) return false;
        x = x * 10 + d;
      }
    }
    *v = x;
    return true;
  }

  // 4 lowercase hex characters -> 2 bytes, the rule of hex8 (host/wire.cpp) on a 32-bit word.  Per character:
  // value = low nibble + 9 if bit 6 is set (letters); valid iff the value is < 16 and maps back to that character.
  __host__ __device__ static uint32_t hex4(uint32_t w, uint32_t* bad) {
    constexpr uint32_t ones = 0x01010101u, high = 0x80808080u;
    // (the products by 9 and 0x27 of the 64-bit original as shifts: every byte of letter and gt9 is 0 or 1)
    const uint32_t letter = (w >> 6) & ones;
    const uint32_t val = (w & (ones * 0x0F)) + letter + (letter << 3);
    const uint32_t gt9 = ((val + ones * 0x76) & high) >> 7;
    const uint32_t recon = val + ones * 0x30 + ((gt9 << 5) | (gt9 << 2) | (gt9 << 1) | gt9);
    *bad |= (recon ^ w) | ((val + ones * 0x70) & high);
    const uint32_t x = ((val & 0x00FF00FFu) << 4) | ((val >> 8) & 0x00FF00FFu);
    return (x | (x >> 8)) & 0xFFFFu;
  }

  // 128 hex characters and the closing quote -> 16 words (64 bytes, in memory order)
  __host__ __device__ bool hex64(uint32_t out[16]) {
    if (p + 129 > e || byte(p + 128) != '"') return false;
    const uint32_t i0 = p >> 2, s = (p & 3) * 8;  // 33 aligned dwords, funnel-shifted
    uint32_t prev = rd.dword(i0), bad = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) {
      const uint32_t mid = rd.dword(i0 + 2 * j + 1), next = rd.dword(i0 + 2 * j + 2);
      const uint32_t w0 = (uint32_t)((((uint64_t)mid << 32) | prev) >> s);
      const uint32_t w1 = (uint32_t)((((uint64_t)next << 32) | mid) >> s);
      out[j] = hex4(w0, &bad) | (hex4(w1, &bad) << 16);
      prev = next;
    }
    if (bad) return false;
    p += 129;
    return true;
  }
};

// One frame: n bytes at row position b0 (< 4).  peer: the connection's authenticated replica, or FRAME_NO_PEER.
// rec: the 160-byte record as 40 words (include/pbft_wire.h): R || S, the 85-byte envelope "PBFT" | kind | view LE |
// seq LE | digest at byte 64, key index LE at byte 150; all zero with key index FRAME_NO_KEY unless the status is OK.
// h: view, seq and kind are set only for OK; key_idx is FRAME_NO_KEY otherwise.  Returns the status.
template <class Rd>
__host__ __device__ inline uint32_t wire_decode_frame(const Rd& rd, uint32_t b0, uint32_t n, uint32_t n_replicas,
                                                      uint32_t peer, uint32_t rec[40], frame_fields& h) {
#pragma unroll
  for (int k = 0; k < 40; ++k) rec[k] = 0;
  rec[37] = FRAME_NO_KEY << 16;
  h.view = h.seq = 0;
  h.kind = 0;
  h.key_idx = FRAME_NO_KEY;
  h.status = WIRE_ST_EDEFER;
  if (n < FRAME_MIN || n > FRAME_MAX) return WIRE_ST_EDEFER;  // decided without reading the body
  frame_cursor<Rd> c{rd, b0, b0 + n};
  uint32_t kind;
  if (c.lit("{\"Prepare\":{\"view\":")) kind = 1;
  else if (c.lit("{\"Commit\":{\"view\":")) kind = 2;
  else return WIRE_ST_EDEFER;
  uint64_t view, seq, rep;
  uint32_t dg[16], sg[16];
  if (!c.num(&view) || !c.lit(",\"sequence_number\":") || !c.num(&seq) || !c.lit(",\"digest\":\"") || !c.hex64(dg) ||
      !c.lit(",\"replica\":") || !c.num(&rep) || rep > 0xFFFFu || !c.lit(",\"signature\":\"") || !c.hex64(sg) ||
      !c.lit("}}") || c.p != c.e)
    return WIRE_ST_EDEFER;
  if (rep >= n_replicas || (peer != FRAME_NO_PEER && (uint32_t)rep != peer)) {
    h.status = WIRE_ST_ESIGNER;
    return WIRE_ST_ESIGNER;
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) rec[k] = sg[k];
  rec[16] = 0x54464250u;  // "PBFT"
  rec[17] = kind | ((uint32_t)view << 8);
  rec[18] = (uint32_t)(view >> 24);
  rec[19] = (uint32_t)(view >> 56) | ((uint32_t)seq << 8);
  rec[20] = (uint32_t)(seq >> 24);
  rec[21] = (uint32_t)(seq >> 56) | (dg[0] << 8);
#pragma unroll
  for (int k = 0; k < 15; ++k) rec[22 + k] = (dg[k] >> 24) | (dg[k + 1] << 8);
  rec[37] = (dg[15] >> 24) | ((uint32_t)rep << 16);
  h.view = view;
  h.seq = seq;
  h.kind = kind;
  h.key_idx = (uint32_t)rep;
  h.status = WIRE_ST_OK;
  return WIRE_ST_OK;
}

// Host accessor: the frame's bytes in memory, presented as a row with the frame at position b0 and `fill` in every
// byte outside it.  Reads no byte outside [p, p + n).
struct frame_mem_reader {
  const uint8_t* p;
  uint32_t b0, n;
  uint8_t fill;
  __host__ __device__ uint32_t dword(uint32_t i) const {
    uint32_t w = 0;
    for (uint32_t b = 0; b < 4; ++b) {
      const uint32_t at = 4 * i + b;
      const uint8_t v = (at >= b0 && at - b0 < n) ? p[at - b0] : fill;
      w |= (uint32_t)v << (8 * b);
    }
    return w;
  }
};

}  // namespace pbft
