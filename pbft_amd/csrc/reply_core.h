// The canonical signed client reply, shared by the host (pbft_wire_encode_replies, pbft_wire_decode_reply, the length
// queries of pbft_sign_replies and pbft_replica_reply) and the device (reply.hip):
//   {"view":V,"timestamp":T,"peer_id":"<52 base58 chars>","result":"R","replica":I,"signature":"<128 hex>"}
// the reference's ClientReply (src/message.rs:54-103) in its field order, followed by the two fields this project adds to
// every signed message.  No varint: the reference writes reply.to_string() raw, one reply per connection
// (src/client_handler.rs:75-84).  A reply is canonical when R is 0 .. RP_RESULT_MAX bytes, all of them in pr_alphabet
// (0x20 .. 0x7E without '"' and '\'): its text needs no escaping and is byte for byte what the general encoder writes.
// The text is head | R | tail: the head is everything in front of R (at most RP_HEAD_MAX bytes), the tail everything
// from `","replica":` on (at most RP_TAIL_MAX).  Its length depends only on the decimal widths of view, timestamp and
// replica and on the result's length.
//
// What is signed is the 85-byte envelope "PBFT" | 3 | view LE | timestamp LE | D with
// D = Blake2b-512(C[64] | R), C the request's 64-byte client field with everything from its first NUL on replaced by
// zeros (rp_client_norm): the serialized reply does not carry the client, so the digest binds it.
//
// rp_match is the reader-side twin: a byte-for-byte matcher of the canonical text.  RP_RH_OK implies that the writer,
// given the fields it answers, writes the same bytes.
#pragma once
#include <stdint.h>

#include "propose_core.h"

namespace pbft {

constexpr uint32_t RP_ST_OK = 0, RP_ST_GENERAL = 1;  // PBFT_REPLY_OK / _GENERAL of include/pbft_wire.h
constexpr uint32_t RP_RH_NONE = 0, RP_RH_OK = 1;     // PBFT_RH_* of include/pbft_wire.h
constexpr uint32_t RP_KIND = 3;                      // PBFT_KIND_REPLY
constexpr uint32_t RP_RESULT_MAX = PR_OP_MAX;        // the copy loop's bound is the one the proposals measured
constexpr uint32_t RP_CLIENT_FIELD = PR_CLIENT_FIELD;
constexpr uint32_t RP_PEER_ID_RAW = 38, RP_PEER_ID_B58 = 52;
constexpr uint32_t RP_MAX_REPLICA = EG_MAX_REPLICA;
constexpr uint64_t RP_MAX_N = (uint64_t)1 << 24;

// The base58btc length of the 38-byte PeerId 00 24 08 01 12 20 | A with every byte of A equal to `fill`: the number of
// base-58 digits of the 37-byte value plus one '1' for the leading zero byte.
constexpr uint32_t rp_b58_len_of(uint8_t fill) {
  uint8_t num[RP_PEER_ID_RAW] = {0x00, 0x24, 0x08, 0x01, 0x12, 0x20};
  for (uint32_t i = 6; i < RP_PEER_ID_RAW; ++i) num[i] = fill;
  uint32_t digits = 0;
  bool nonzero = true;
  while (nonzero) {
    uint32_t rem = 0;
    nonzero = false;
    for (uint32_t i = 0; i < RP_PEER_ID_RAW; ++i) {
      const uint32_t cur = rem * 256 + num[i];
      num[i] = (uint8_t)(cur / 58);
      rem = cur % 58;
      nonzero = nonzero || num[i] != 0;
    }
    ++digits;
  }
  return digits + 1;
}
// The value lies in [0x24 * 256^36, 0x25 * 256^36) whatever A is, and both ends have 51 base-58 digits.
static_assert(rp_b58_len_of(0x00) == RP_PEER_ID_B58 && rp_b58_len_of(0xFF) == RP_PEER_ID_B58,
              "an Ed25519 PeerId's base58btc text always has 52 characters");

#define PBFT_RP_L0 "{\"view\":"
#define PBFT_RP_L1 ",\"timestamp\":"
#define PBFT_RP_L2 ",\"peer_id\":\""
#define PBFT_RP_L3 "\",\"result\":\""
#define PBFT_RP_L4 "\",\"replica\":"
#define PBFT_RP_L5 ",\"signature\":\""
#define PBFT_RP_L6 "\"}"
#define PBFT_RP_B58 "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"
constexpr uint32_t RP_HEAD_FIXED = (uint32_t)(sizeof(PBFT_RP_L0 PBFT_RP_L1 PBFT_RP_L2 PBFT_RP_L3) - 1) + RP_PEER_ID_B58;
constexpr uint32_t RP_TAIL_FIXED = (uint32_t)(sizeof(PBFT_RP_L4 PBFT_RP_L5 PBFT_RP_L6) - 1) + 128;
constexpr uint32_t RP_HEAD_MAX = RP_HEAD_FIXED + 2 * 20;
constexpr uint32_t RP_TAIL_MAX = RP_TAIL_FIXED + 5;
constexpr uint32_t RP_TEXT_MIN = RP_HEAD_FIXED + 2 + RP_TAIL_FIXED + 1;
constexpr uint32_t RP_TEXT_MAX = RP_HEAD_MAX + RP_RESULT_MAX + RP_TAIL_MAX;
static_assert(RP_HEAD_FIXED == 97 && RP_HEAD_MAX == 137, "the head of the longest reply");
static_assert(RP_TAIL_FIXED == 156 && RP_TAIL_MAX == 161, "the tail of the longest reply");
static_assert(RP_TEXT_MIN == 256 && RP_TEXT_MAX == 298 + RP_RESULT_MAX, "the reply's length window");

// C: the client field up to its first NUL, zeros behind it (a field without a NUL is taken whole).
EG_FN void rp_client_norm(uint8_t out[RP_CLIENT_FIELD], const uint8_t* field) {
  bool open = true;
  for (uint32_t k = 0; k < RP_CLIENT_FIELD; ++k) {
    const uint8_t b = field[k];
    open = open && b != 0;
    out[k] = open ? b : (uint8_t)0;
  }
}

// Canonical or not, from the length and the bytes (the result is not touched unless its length is in range).
EG_FN bool rp_canonical(const uint8_t* res, uint32_t res_len) {
  return res_len <= RP_RESULT_MAX && pr_all_alphabet(res, res_len);
}

EG_FN uint32_t rp_head_len(uint64_t view, uint64_t timestamp) {
  return RP_HEAD_FIXED + eg_dec_width(view) + eg_dec_width(timestamp);
}
EG_FN uint32_t rp_tail_len(uint32_t replica) { return RP_TAIL_FIXED + eg_dec_width(replica); }
// Bytes of a canonical reply's text.
EG_FN uint32_t rp_text_len(uint64_t view, uint64_t timestamp, uint32_t replica, uint32_t res_len) {
  return rp_head_len(view, timestamp) + res_len + rp_tail_len(replica);
}

// Sink: void operator()(uint32_t pos, uint8_t byte).  The head at positions [0, rp_head_len): everything in front of R;
// peer_id: the 52 characters.  Returns its length.
template <class Sink>
EG_FN uint32_t rp_write_head(Sink& put, uint64_t view, uint64_t timestamp, const uint8_t* peer_id) {
  uint32_t p = 0;
  p = eg_put_lit(put, p, PBFT_RP_L0, (uint32_t)sizeof(PBFT_RP_L0) - 1);
  p = eg_put_dec(put, p, view);
  p = eg_put_lit(put, p, PBFT_RP_L1, (uint32_t)sizeof(PBFT_RP_L1) - 1);
  p = eg_put_dec(put, p, timestamp);
  p = eg_put_lit(put, p, PBFT_RP_L2, (uint32_t)sizeof(PBFT_RP_L2) - 1);
  for (uint32_t i = 0; i < RP_PEER_ID_B58; ++i) put(p + i, peer_id[i]);
  p += RP_PEER_ID_B58;
  p = eg_put_lit(put, p, PBFT_RP_L3, (uint32_t)sizeof(PBFT_RP_L3) - 1);
  return p;
}

// The tail at positions [pos, pos + rp_tail_len): from `","replica":` on; sig = R || S as 16 little-endian words.
// Returns the position behind it.
template <class Sink>
EG_FN uint32_t rp_write_tail(Sink& put, uint32_t pos, uint32_t replica, const uint32_t sig[16]) {
  uint32_t p = pos;
  p = eg_put_lit(put, p, PBFT_RP_L4, (uint32_t)sizeof(PBFT_RP_L4) - 1);
  p = eg_put_dec(put, p, replica);
  p = eg_put_lit(put, p, PBFT_RP_L5, (uint32_t)sizeof(PBFT_RP_L5) - 1);
  p = eg_put_hex_words(put, p, sig, 16);
  p = eg_put_lit(put, p, PBFT_RP_L6, (uint32_t)sizeof(PBFT_RP_L6) - 1);
  return p;
}

// The whole text of a canonical reply; returns its length, rp_text_len of the same fields.
template <class Sink>
EG_FN uint32_t rp_write_text(Sink& put, uint64_t view, uint64_t timestamp, const uint8_t* peer_id, const uint8_t* res,
                             uint32_t res_len, uint32_t replica, const uint32_t sig[16]) {
  const uint32_t p = rp_write_head(put, view, timestamp, peer_id);
  for (uint32_t i = 0; i < res_len; ++i) put(p + i, res[i]);
  return rp_write_tail(put, p + res_len, replica, sig);
}

// ---- the reader-side twin ----
struct rp_head {
  uint64_t view, timestamp;
  uint32_t result_off, result_len, replica, status;
  uint8_t peer_id[RP_PEER_ID_B58];
  uint8_t sig[64];
};

EG_FN bool rp_m_lit(const uint8_t* t, uint32_t n, uint32_t& p, const char* s, uint32_t k) {
  if (n - p < k) return false;
  for (uint32_t i = 0; i < k; ++i)
    if (t[p + i] != (uint8_t)s[i]) return false;
  p += k;
  return true;
}
// A u64 as the writer prints it: 1 .. 20 digits, no leading zero, no overflow; at most `max`.
EG_FN bool rp_m_dec(const uint8_t* t, uint32_t n, uint32_t& p, uint64_t max, uint64_t& v) {
  uint32_t k = 0;
  v = 0;
  while (p + k < n && k < 20 && t[p + k] >= '0' && t[p + k] <= '9') {
    const uint64_t d = (uint64_t)(t[p + k] - '0');
    if (v > (~(uint64_t)0 - d) / 10) return false;
    v = v * 10 + d;
    ++k;
  }
  if (k == 0 || (k > 1 && t[p] == '0') || v > max) return false;
  if (p + k < n && t[p + k] >= '0' && t[p + k] <= '9') return false;  // a 21st digit
  p += k;
  return true;
}
EG_FN bool rp_m_hexval(uint32_t c, uint32_t& v) {
  if (c >= '0' && c <= '9') v = c - '0';
  else if (c >= 'a' && c <= 'f') v = c - 'a' + 10;
  else return false;
  return true;
}
EG_FN bool rp_b58_char(uint32_t c) {
  const char* a = PBFT_RP_B58;
  for (uint32_t i = 0; i < 58; ++i)
    if ((uint32_t)(uint8_t)a[i] == c) return true;
  return false;
}

// The text t[0, n) against the canonical form.  h.status = RP_RH_OK and every field set, or RP_RH_NONE (fields
// unspecified).  Every byte read lies in [t, t + n).
EG_FN uint32_t rp_match(const uint8_t* t, uint64_t n64, rp_head& h) {
  h.status = RP_RH_NONE;
  if (n64 < RP_TEXT_MIN || n64 > RP_TEXT_MAX) return RP_RH_NONE;
  const uint32_t n = (uint32_t)n64;
  uint32_t p = 0;
  uint64_t rep = 0;
  if (!rp_m_lit(t, n, p, PBFT_RP_L0, (uint32_t)sizeof(PBFT_RP_L0) - 1)) return RP_RH_NONE;
  if (!rp_m_dec(t, n, p, ~(uint64_t)0, h.view)) return RP_RH_NONE;
  if (!rp_m_lit(t, n, p, PBFT_RP_L1, (uint32_t)sizeof(PBFT_RP_L1) - 1)) return RP_RH_NONE;
  if (!rp_m_dec(t, n, p, ~(uint64_t)0, h.timestamp)) return RP_RH_NONE;
  if (!rp_m_lit(t, n, p, PBFT_RP_L2, (uint32_t)sizeof(PBFT_RP_L2) - 1)) return RP_RH_NONE;
  if (n - p < RP_PEER_ID_B58) return RP_RH_NONE;
  for (uint32_t i = 0; i < RP_PEER_ID_B58; ++i) {
    if (!rp_b58_char(t[p + i])) return RP_RH_NONE;
    h.peer_id[i] = t[p + i];
  }
  p += RP_PEER_ID_B58;
  if (!rp_m_lit(t, n, p, PBFT_RP_L3, (uint32_t)sizeof(PBFT_RP_L3) - 1)) return RP_RH_NONE;
  h.result_off = p;
  uint32_t k = 0;
  while (p + k < n && k <= RP_RESULT_MAX && pr_alphabet(t[p + k])) ++k;
  if (k > RP_RESULT_MAX) return RP_RH_NONE;
  h.result_len = k;
  p += k;  // (the closing quote, if that is what stopped the scan, opens the tail)
  if (!rp_m_lit(t, n, p, PBFT_RP_L4, (uint32_t)sizeof(PBFT_RP_L4) - 1)) return RP_RH_NONE;
  if (!rp_m_dec(t, n, p, RP_MAX_REPLICA, rep)) return RP_RH_NONE;
  h.replica = (uint32_t)rep;
  if (!rp_m_lit(t, n, p, PBFT_RP_L5, (uint32_t)sizeof(PBFT_RP_L5) - 1)) return RP_RH_NONE;
  if (n - p < 128) return RP_RH_NONE;
  for (uint32_t i = 0; i < 64; ++i) {
    uint32_t hi = 0, lo = 0;
    if (!rp_m_hexval(t[p + 2 * i], hi) || !rp_m_hexval(t[p + 2 * i + 1], lo)) return RP_RH_NONE;
    h.sig[i] = (uint8_t)(hi << 4 | lo);
  }
  p += 128;
  if (!rp_m_lit(t, n, p, PBFT_RP_L6, (uint32_t)sizeof(PBFT_RP_L6) - 1)) return RP_RH_NONE;
  if (p != n) return RP_RH_NONE;  // a trailing byte
  h.status = RP_RH_OK;
  return RP_RH_OK;
}

// The PeerId text of the Ed25519 key A: base58btc of 00 24 08 01 12 20 | A, always RP_PEER_ID_B58 characters (host side:
// computed once per installed seed; there is no base58 on the device).  Returns the number of characters, which the
// callers check against RP_PEER_ID_B58.
inline uint32_t rp_peer_id_b58(const uint8_t A[32], uint8_t out[RP_PEER_ID_B58]) {
  static const char alpha[] = PBFT_RP_B58;
  uint8_t num[RP_PEER_ID_RAW] = {0x00, 0x24, 0x08, 0x01, 0x12, 0x20};
  for (uint32_t i = 0; i < 32; ++i) num[6 + i] = A[i];
  uint8_t digits[RP_PEER_ID_B58 + 4];
  uint32_t nd = 0;
  bool nonzero = true;
  while (nonzero && nd < RP_PEER_ID_B58 + 3) {
    uint32_t rem = 0;
    nonzero = false;
    for (uint32_t i = 0; i < RP_PEER_ID_RAW; ++i) {
      const uint32_t cur = rem * 256 + num[i];
      num[i] = (uint8_t)(cur / 58);
      rem = cur % 58;
      nonzero = nonzero || num[i] != 0;
    }
    digits[nd++] = (uint8_t)rem;
  }
  const uint32_t total = nd + 1;  // one '1' for the leading zero byte
  if (total != RP_PEER_ID_B58) return total;
  out[0] = '1';
  for (uint32_t i = 0; i < nd; ++i) out[1 + i] = (uint8_t)alpha[digits[nd - 1 - i]];
  return total;
}

#undef PBFT_RP_L0
#undef PBFT_RP_L1
#undef PBFT_RP_L2
#undef PBFT_RP_L3
#undef PBFT_RP_L4
#undef PBFT_RP_L5
#undef PBFT_RP_L6
#undef PBFT_RP_B58

}  // namespace pbft
