// The canonical signed PrePrepare frame written from a client request, shared by the host (pbft_wire_encode_preprepares,
// the length queries of pbft_sign_preprepares_frames and pbft_replica_propose) and the device (propose.hip):
//   varint(len) {"PrePrepare":{"view":V,"sequence_number":N,"digest":"<128 hex>","message":{"operation":"OP",
//   "timestamp":T,"client":"C"},"replica":R,"signature":"<128 hex>"}}
// the writer-side twin of wire_pp_core.h: a request is canonical when OP is 0 .. PR_OP_MAX bytes and C (its 64-byte
// field up to the first NUL) 1 .. PR_CLIENT_MAX bytes, all of them in pr_alphabet (0x20 .. 0x7E without '"' and '\').
// Such a frame needs no escaping, is byte for byte what pbft_wire_encode_frame writes (host/wire.cpp), and is exactly
// what wire_pp_frame accepts.  Its length depends only on the decimal widths of view, seq, timestamp and replica, on
// op_len and on client_len; the body is PR_BODY_MIN .. PR_BODY_MAX bytes (PBFT_PP_FRAME_MIN .. _MAX), so its varint
// always has two bytes.  The frame is head | OP | tail: the head is everything in front of OP (at most PR_HEAD_MAX
// bytes, varint included), the tail everything from `","timestamp":` on (at most PR_TAIL_MAX).
//
// The digest on the device: blake2b512_span (sign_tile.h) is Blake2b-512 (digest_kernels.h's compression) over the
// operation where it lies, read through aligned dwords (digest_kernels.h's le64_masked may load the dword behind the
// operation's last one; this reader does not).  An aligned dword is loaded only if at least one of its four bytes belongs to the operation,
// and the bytes of it that do not are masked off.  For an operation inside [ops, ops + ops_bytes) with ops 4-byte
// aligned, every byte read therefore lies in [ops, round_up(ops_bytes, 4)), inside the 16-byte rule of the entry points.
#pragma once
#include <stdint.h>

#include "egress_core.h"

namespace pbft {

constexpr uint32_t PR_ST_OK = 0, PR_ST_GENERAL = 1;  // PBFT_PROPOSE_* of include/pbft_wire.h
constexpr uint32_t PR_OP_MAX = 3072, PR_CLIENT_MAX = 63, PR_CLIENT_FIELD = 64;
constexpr uint32_t PR_MAX_REPLICA = EG_MAX_REPLICA;
constexpr uint64_t PR_MAX_N = (uint64_t)1 << 24;

#define PBFT_PR_L0 "{\"PrePrepare\":{\"view\":"
#define PBFT_PR_L1 ",\"sequence_number\":"
#define PBFT_PR_L2 ",\"digest\":\""
#define PBFT_PR_L3 "\",\"message\":{\"operation\":\""
#define PBFT_PR_L4 "\",\"timestamp\":"
#define PBFT_PR_L5 ",\"client\":\""
#define PBFT_PR_L6 "\"},\"replica\":"
#define PBFT_PR_L7 ",\"signature\":\""
#define PBFT_PR_L8 "\"}}"
constexpr uint32_t PR_HEAD_FIXED = 2 + (uint32_t)(sizeof(PBFT_PR_L0 PBFT_PR_L1 PBFT_PR_L2 PBFT_PR_L3) - 1) + 128;
constexpr uint32_t PR_TAIL_FIXED = (uint32_t)(sizeof(PBFT_PR_L4 PBFT_PR_L5 PBFT_PR_L6 PBFT_PR_L7 PBFT_PR_L8) - 1) + 128;
constexpr uint32_t PR_HEAD_MAX = PR_HEAD_FIXED + 2 * 20;
constexpr uint32_t PR_TAIL_MAX = PR_TAIL_FIXED + 20 + PR_CLIENT_MAX + 5;
constexpr uint32_t PR_BODY_MIN = PR_HEAD_FIXED - 2 + PR_TAIL_FIXED + 2 + 0 + 1 + 1 + 1;
constexpr uint32_t PR_BODY_MAX = PR_HEAD_MAX - 2 + PR_OP_MAX + PR_TAIL_MAX;
constexpr uint32_t PR_FRAME_MAX = PR_BODY_MAX + 2;  // with the two-byte varint
static_assert(PR_HEAD_MAX == 248 && PR_TAIL_MAX == 271, "the head and the tail of the longest frame");
static_assert(PR_BODY_MIN == 394 && PR_BODY_MAX == 517 + PR_OP_MAX, "the PrePrepare's length window");
static_assert(PR_BODY_MIN >= 128 && PR_BODY_MAX < 16384, "a two-byte varint");
#if defined(PBFT_PP_OP_MAX)  // include/pbft_wire.h, where it is in sight
static_assert(PR_OP_MAX == PBFT_PP_OP_MAX && PR_BODY_MIN == PBFT_PP_FRAME_MIN && PR_BODY_MAX == PBFT_PP_FRAME_MAX,
              "the writer's limits are the ingress matcher's");
#endif

EG_FN bool pr_alphabet(uint32_t c) { return c >= 0x20u && c <= 0x7Eu && c != '"' && c != '\\'; }

// The client's length: up to the first NUL of its 64-byte field (64: no NUL).
EG_FN uint32_t pr_client_len(const uint8_t* c) {
  uint32_t n = 0;
  while (n < PR_CLIENT_FIELD && c[n]) ++n;
  return n;
}

// One byte string against the alphabet, eight bytes per step (exactly the string's bytes are read).  Per 8-byte word
// w, a set top bit in `bad` marks: a byte >= 0x80; one below 0x20 (b + 0x60 stays below 0x80) or equal to 0x7F
// (b + 1 reaches 0x80), tested on the low seven bits so that no sum carries into the next byte; a byte equal to '"'
// or '\' (the zero byte of w ^ 0x22.. / w ^ 0x5C..: (x - 0x01..) & ~x has its top bit set in the lowest zero byte,
// and in no byte when there is none).
EG_FN bool pr_all_alphabet(const uint8_t* p, uint32_t n) {
  const uint64_t K01 = 0x0101010101010101ull, K80 = 0x8080808080808080ull;
  uint64_t bad = 0;
  uint32_t i = 0;
  for (; i + 8 <= n; i += 8) {
    uint64_t w;
    __builtin_memcpy(&w, p + i, 8);
    const uint64_t low = w & ~K80, q = w ^ (0x22 * K01), s = w ^ (0x5C * K01);
    bad |= w | ~(low + 0x60 * K01) | (low + K01) | ((q - K01) & ~q) | ((s - K01) & ~s);
  }
  uint32_t tail = 0;
  for (; i < n; ++i) tail |= (uint32_t)!pr_alphabet(p[i]);
  return (bad & K80) == 0 && tail == 0;
}

// Canonical or not, from the lengths and the bytes (op is not touched unless its length is in range).
EG_FN bool pr_canonical(const uint8_t* op, uint32_t op_len, const uint8_t* client, uint32_t client_len) {
  if (op_len > PR_OP_MAX || client_len < 1 || client_len > PR_CLIENT_MAX) return false;
  return pr_all_alphabet(client, client_len) && pr_all_alphabet(op, op_len);
}

EG_FN uint32_t pr_head_len(uint64_t view, uint64_t seq) { return PR_HEAD_FIXED + eg_dec_width(view) + eg_dec_width(seq); }
EG_FN uint32_t pr_tail_len(uint64_t timestamp, uint32_t client_len, uint32_t replica) {
  return PR_TAIL_FIXED + eg_dec_width(timestamp) + client_len + eg_dec_width(replica);
}
// Bytes of a canonical request's frame, varint included.
EG_FN uint32_t pr_frame_len(uint64_t view, uint64_t seq, uint64_t timestamp, uint32_t replica, uint32_t op_len,
                            uint32_t client_len) {
  return pr_head_len(view, seq) + op_len + pr_tail_len(timestamp, client_len, replica);
}

// Sink: void operator()(uint32_t pos, uint8_t byte).  The head at positions [0, pr_head_len): the varint of the whole
// body (frame_len - 2) and everything in front of OP; digest as 16 little-endian words.  Returns its length.
template <class Sink>
EG_FN uint32_t pr_write_head(Sink& put, uint32_t frame_len, uint64_t view, uint64_t seq, const uint32_t digest[16]) {
  const uint32_t body = frame_len - 2;
  put(0, (uint8_t)(0x80 | (body & 0x7F)));
  put(1, (uint8_t)(body >> 7));
  uint32_t p = 2;
  p = eg_put_lit(put, p, PBFT_PR_L0, (uint32_t)sizeof(PBFT_PR_L0) - 1);
  p = eg_put_dec(put, p, view);
  p = eg_put_lit(put, p, PBFT_PR_L1, (uint32_t)sizeof(PBFT_PR_L1) - 1);
  p = eg_put_dec(put, p, seq);
  p = eg_put_lit(put, p, PBFT_PR_L2, (uint32_t)sizeof(PBFT_PR_L2) - 1);
  p = eg_put_hex_words(put, p, digest, 16);
  p = eg_put_lit(put, p, PBFT_PR_L3, (uint32_t)sizeof(PBFT_PR_L3) - 1);
  return p;
}

// The tail at positions [pos, pos + pr_tail_len): from `","timestamp":` on; sig = R || S as 16 little-endian words.
// Returns the position behind it.
template <class Sink>
EG_FN uint32_t pr_write_tail(Sink& put, uint32_t pos, uint64_t timestamp, const uint8_t* client, uint32_t client_len,
                             uint32_t replica, const uint32_t sig[16]) {
  uint32_t p = pos;
  p = eg_put_lit(put, p, PBFT_PR_L4, (uint32_t)sizeof(PBFT_PR_L4) - 1);
  p = eg_put_dec(put, p, timestamp);
  p = eg_put_lit(put, p, PBFT_PR_L5, (uint32_t)sizeof(PBFT_PR_L5) - 1);
  for (uint32_t i = 0; i < client_len; ++i) put(p + i, client[i]);
  p += client_len;
  p = eg_put_lit(put, p, PBFT_PR_L6, (uint32_t)sizeof(PBFT_PR_L6) - 1);
  p = eg_put_dec(put, p, replica);
  p = eg_put_lit(put, p, PBFT_PR_L7, (uint32_t)sizeof(PBFT_PR_L7) - 1);
  p = eg_put_hex_words(put, p, sig, 16);
  p = eg_put_lit(put, p, PBFT_PR_L8, (uint32_t)sizeof(PBFT_PR_L8) - 1);
  return p;
}

// The whole frame of a canonical request; returns its length, pr_frame_len of the same fields.
template <class Sink>
EG_FN uint32_t pr_write_frame(Sink& put, uint64_t view, uint64_t seq, const uint32_t digest[16], const uint8_t* op,
                              uint32_t op_len, uint64_t timestamp, const uint8_t* client, uint32_t client_len,
                              uint32_t replica, const uint32_t sig[16]) {
  const uint32_t len = pr_frame_len(view, seq, timestamp, replica, op_len, client_len);
  uint32_t p = pr_write_head(put, len, view, seq, digest);
  for (uint32_t i = 0; i < op_len; ++i) put(p + i, op[i]);
  return pr_write_tail(put, p + op_len, timestamp, client, client_len, replica, sig);
}

#undef PBFT_PR_L0
#undef PBFT_PR_L1
#undef PBFT_PR_L2
#undef PBFT_PR_L3
#undef PBFT_PR_L4
#undef PBFT_PR_L5
#undef PBFT_PR_L6
#undef PBFT_PR_L7
#undef PBFT_PR_L8

}  // namespace pbft
