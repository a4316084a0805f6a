// The canonical signed PrePrepare, shared by the host (pbft_wire_decode_preprepare) and the device (wire_pp.hip):
//   {"PrePrepare":{"view":V,"sequence_number":N,"digest":"<128 hex>","message":{"operation":"OP","timestamp":T,
//   "client":"C"},"replica":R,"signature":"<128 hex>"}}
// exactly what pbft_wire_encode_json writes (host/wire.cpp), matched byte for byte with wire_decode_core.h's cursor.
// Accepted only when V, N and T are serde u64 (digits, no leading zero, no overflow), R <= 65535, both hex strings are
// 128 lowercase digits, OP is 0 .. PP_OP_MAX bytes and C 1 .. 63 bytes of 0x20 .. 0x7E without '"' and '\' (so there is
// no escape, no control byte and no UTF-8 to validate), and nothing follows "}}".  Whatever is not that form is
// PP_ST_NONE and the general parser decides, with serde's rules.  The contract is one-sided, as fast_vote's: PP_ST_OK
// implies that pbft_wire_decode_json accepts the frame as a PrePrepare with digest_ok and has_sig, with these fields
// and an operation equal to bytes [op_off, op_off + op_len) of the body.
//
// The frame is read through wire_decode_core.h's accessor of aligned dwords (the frame occupies bytes [b0, b0 + n) of a
// row; here b0 < 16 and the row has PP_ROW_DWORDS dwords) and through a scanner for the two free strings,
//   uint32_t Scan::operator()(uint32_t from, uint32_t limit) const
// = the row position of the first byte in [from, limit) outside the alphabet, or limit.  The host walks bytes; the
// kernel gives every lane a dword and takes a ballot, which is why its whole wave runs this function in step.
//
// The digest: pp_digest is blake2b512 (digest_kernels.h) over the operation where it lies.  le64_masked asks for at most
// 3 bytes past op_len, through load_u32_unaligned's two covering aligned dwords: bytes from 3 in front of the operation
// to 6 behind it may be touched.  In front of it lie >= 206 bytes of the same frame, behind it `","timestamp":` and
// >= 169 more: never a byte outside the frame.
#pragma once
#include "digest_kernels.h"
#include "wire_decode_core.h"

namespace pbft {

constexpr uint32_t PP_ST_NONE = 0, PP_ST_OK = 1;  // PBFT_PP_* of include/pbft_wire.h
constexpr uint32_t PP_OP_MAX = 3072, PP_CLIENT_MAX = 63;

#define PBFT_PP_L0 "{\"PrePrepare\":{\"view\":"
#define PBFT_PP_L1 ",\"sequence_number\":"
#define PBFT_PP_L2 ",\"digest\":\""
#define PBFT_PP_L3 ",\"message\":{\"operation\":\""
#define PBFT_PP_L4 "\",\"timestamp\":"
#define PBFT_PP_L5 ",\"client\":\""
#define PBFT_PP_L6 "\"},\"replica\":"
#define PBFT_PP_L7 ",\"signature\":\""
#define PBFT_PP_L8 "}}"
// the skeleton: the nine literals, two hex strings and their closing quotes
constexpr uint32_t PP_SKELETON =
    (uint32_t)(sizeof(PBFT_PP_L0 PBFT_PP_L1 PBFT_PP_L2 PBFT_PP_L3 PBFT_PP_L4 PBFT_PP_L5 PBFT_PP_L6 PBFT_PP_L7 PBFT_PP_L8) -
               1) + 2 * 129;
constexpr uint32_t PP_FRAME_MIN = PP_SKELETON + 3 + 0 + 1 + 1;                           // one-digit numbers, "" and "C"
constexpr uint32_t PP_FRAME_MAX = PP_SKELETON + 3 * 20 + PP_OP_MAX + PP_CLIENT_MAX + 5;  // 20-digit numbers, 65535
// a frame that starts anywhere in a 16-byte granule: ceil((15 + PP_FRAME_MAX) / 16) granules, and one more, so that
// the cursor's reads of the dword behind the one it needs stay inside the row
constexpr uint32_t PP_ROW_GRANULES = (15 + PP_FRAME_MAX + 15) / 16 + 1;
constexpr uint32_t PP_ROW_DWORDS = 4 * PP_ROW_GRANULES;

struct pp_fields {
  uint64_t view, seq, timestamp;
  uint32_t op_off, op_len, replica, status;  // op_off counts from the body's first byte
  uint32_t claimed[16], sig[16];             // 64 bytes each, in memory order
};

__host__ __device__ inline bool pp_alphabet(uint32_t c) { return c >= 0x20u && c <= 0x7Eu && c != '"' && c != '\\'; }

// One frame: n bytes at row position b0.  h is all zero unless the status is PP_ST_OK.  Returns the status.
template <class Rd, class Scan>
__host__ __device__ inline uint32_t wire_pp_frame(const Rd& rd, const Scan& scan, uint32_t b0, uint32_t n, pp_fields& h) {
  h.view = h.seq = h.timestamp = 0;
  h.op_off = h.op_len = h.replica = 0;
  h.status = PP_ST_NONE;
#pragma unroll
  for (int k = 0; k < 16; ++k) h.claimed[k] = h.sig[k] = 0;
  if (n < PP_FRAME_MIN || n > PP_FRAME_MAX) return PP_ST_NONE;  // decided without reading the body
  frame_cursor<Rd> c{rd, b0, b0 + n};
  if (!c.lit(PBFT_PP_L0)) return PP_ST_NONE;  // (a vote of the right length leaves here)
  uint64_t view, seq, ts, rep;
  uint32_t dg[16], sg[16];
  if (!c.num(&view) || !c.lit(PBFT_PP_L1) || !c.num(&seq) || !c.lit(PBFT_PP_L2) || !c.hex64(dg) || !c.lit(PBFT_PP_L3))
    return PP_ST_NONE;
  // OP: its closing quote is the first byte outside the alphabet, at most PP_OP_MAX bytes on
  const uint32_t op = c.p;
  const uint32_t op_lim = c.e - op > PP_OP_MAX + 1 ? op + PP_OP_MAX + 1 : c.e;
  const uint32_t op_end = scan(op, op_lim);
  if (op_end >= op_lim) return PP_ST_NONE;
  c.p = op_end;  // (L4 begins with the quote: any other stop byte fails it)
  if (!c.lit(PBFT_PP_L4) || !c.num(&ts) || !c.lit(PBFT_PP_L5)) return PP_ST_NONE;
  const uint32_t cl = c.p;
  const uint32_t cl_lim = c.e - cl > PP_CLIENT_MAX + 1 ? cl + PP_CLIENT_MAX + 1 : c.e;
  const uint32_t cl_end = scan(cl, cl_lim);
  if (cl_end >= cl_lim || cl_end == cl) return PP_ST_NONE;
  c.p = cl_end;
  if (!c.lit(PBFT_PP_L6) || !c.num(&rep) || rep > 0xFFFFu || !c.lit(PBFT_PP_L7) || !c.hex64(sg) || !c.lit(PBFT_PP_L8) ||
      c.p != c.e)
    return PP_ST_NONE;
  h.view = view;
  h.seq = seq;
  h.timestamp = ts;
  h.op_off = op - b0;
  h.op_len = op_end - op;
  h.replica = (uint32_t)rep;
  h.status = PP_ST_OK;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    h.claimed[k] = dg[k];
    h.sig[k] = sg[k];
  }
  return PP_ST_OK;
}

#undef PBFT_PP_L0
#undef PBFT_PP_L1
#undef PBFT_PP_L2
#undef PBFT_PP_L3
#undef PBFT_PP_L4
#undef PBFT_PP_L5
#undef PBFT_PP_L6
#undef PBFT_PP_L7
#undef PBFT_PP_L8

// Host scanner: one byte at a time through the accessor.
template <class Rd>
struct pp_byte_scan {
  const Rd& rd;
  __host__ __device__ uint32_t operator()(uint32_t from, uint32_t limit) const {
    for (uint32_t at = from; at < limit; ++at)
      if (!pp_alphabet((rd.dword(at >> 2) >> ((at & 3) * 8)) & 0xFFu)) return at;
    return limit;
  }
};

// Blake2b-512 of the operation where it lies (the bound on what is read: the head of this file).
__host__ __device__ inline void pp_digest(uint8_t out[64], const uint8_t* body, uint32_t op_off, uint32_t op_len) {
  blake2b512(out, body + op_off, op_len);
}

}  // namespace pbft
