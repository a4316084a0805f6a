// The client's acceptance rule, shared by the host (pbft_accept_replies' settlement, tests/native/accept_main.cpp) and
// the device (accept.hip): signed replies in, one 160-byte verifier record and one 32-byte head per reply out.
//
// A reply is the text reply_core.h defines.  It arrives raw on an unauthenticated connection, so its signer is what the
// text claims and the signature is the authentication: "replica":I must be below the installed key count and "peer_id"
// must be, byte for byte, the 52-character PeerId text of installed key I.  The status of reply i, in this order:
//   AC_EDEFER   the text is not canonical (rp_match of reply_core.h answers RP_RH_NONE), or does not lie inside the
//               batch's bytes (then it is not read)
//   AC_ESIGNER  replica out of range, or the peer id is not that key's
//   AC_ECLIENT  client_idx[i] >= n_clients (decided before any address of the client table is formed)
//   AC_OK       none of these
// The record of an OK reply is R | S from the hex, pbft_reply_envelope(view, timestamp, D) with
// D = Blake2b-512(C | result) (C: the client's 64-byte field, normalised by rp_client_norm) and key index I; every other
// reply has the all-zero record with key index 0xFFFF, which grouping, verification and tally skip.
//
// Two replies match iff their 85-byte kind-3 envelopes are equal: the same view, timestamp, client field and result
// bytes.  The view is in the match: replies of different views do not combine.  The reference's view is constant and
// view change is out of scope.
//
// ac_match_frame is rp_match read from both ends: the head is matched forwards from the text's first byte, the tail
// (fixed length but for the replica's 1 .. 5 digits) backwards from its last, and what lies between is the result, whose
// bytes the caller tests against pr_alphabet.  rp_match scans the result forwards up to the first byte outside the
// alphabet and expects the tail there; the tail begins with '"', which is outside the alphabet, so a text passes one
// exactly when it passes the other, with the same fields (tests/native/accept_main.cpp compares them over the corpus,
// its truncations and its single-byte mutations; tests/test_gpu_accept.py does on the device).
#pragma once
#include <stdint.h>

#include "reply_core.h"

namespace pbft {

constexpr uint32_t AC_OK = 0, AC_EDEFER = 1, AC_ESIGNER = 2, AC_ECLIENT = 3, AC_EJSON = 4;  // PBFT_ACCEPT_*
constexpr uint32_t AC_ESCAPED = 0x100;        // PBFT_ACCEPT_ESCAPED: a flag beside AC_OK, host settlement only
constexpr uint32_t AC_NO_KEY = 0xFFFF;        // the key index of a record that is skipped
constexpr uint32_t AC_NO_REPLY = 0xFFFFFFFFu; // accept_cert::first of an envelope without a valid reply
constexpr uint64_t AC_MAX_N = RP_MAX_N;
constexpr uint64_t AC_MAX_TEXT_BYTES = (uint64_t)1 << 31;
// What the matcher reads of a text of n bytes: [0, AC_HEAD_WIN) and [n - AC_TAIL_WIN, n) (n >= RP_TEXT_MIN covers both)
constexpr uint32_t AC_HEAD_WIN = 140, AC_TAIL_WIN = 164;
static_assert(AC_HEAD_WIN >= RP_HEAD_MAX + 1 && AC_TAIL_WIN >= RP_TAIL_MAX + 2 && RP_TEXT_MIN >= AC_TAIL_WIN, "");

struct accept_head {  // pbft_accept_head
  uint64_t view, timestamp;
  uint32_t result_off, result_len;  // the result's bytes, counted from the text's first byte
  uint32_t replica;
  uint32_t status;
};
static_assert(sizeof(accept_head) == 32, "four 8-byte stores");

struct accept_cert {  // pbft_accept_cert
  uint64_t view, timestamp;
  uint32_t first, count, client, accepted;
};
static_assert(sizeof(accept_cert) == 32, "");

struct accept_frame {
  uint64_t view, timestamp;
  uint32_t result_off, result_len, replica;
  uint32_t pid_off;  // where the 52 characters of the peer id stand
};

EG_FN bool ac_digit(uint32_t c) { return c >= '0' && c <= '9'; }
// The base58btc alphabet: 1-9, A-Z without I and O, a-z without l (rp_b58_char's table as ranges)
EG_FN bool ac_b58_char(uint32_t c) {
  return (c >= '1' && c <= '9') || (c >= 'A' && c <= 'Z' && c != 'I' && c != 'O') ||
         (c >= 'a' && c <= 'z' && c != 'l');
}
template <class Rd>
EG_FN bool ac_lit(const Rd& rd, uint32_t n, uint32_t& p, const char* s, uint32_t k) {
  if (n - p < k) return false;
  bool ok = true;
  for (uint32_t i = 0; i < k; ++i) ok = ok && rd(p + i) == (uint32_t)(uint8_t)s[i];
  p += k;
  return ok;
}
// rp_m_dec: 1 .. 20 digits, no leading zero, no overflow, no 21st digit
template <class Rd>
EG_FN bool ac_dec(const Rd& rd, uint32_t n, uint32_t& p, uint64_t& v) {
  uint32_t k = 0;
  v = 0;
  while (p + k < n && k < 20 && ac_digit(rd(p + k))) {
    const uint64_t d = (uint64_t)(rd(p + k) - '0');
    if (v > (~(uint64_t)0 - d) / 10) return false;
    v = v * 10 + d;
    ++k;
  }
  if (k == 0 || (k > 1 && rd(p) == '0')) return false;
  if (p + k < n && ac_digit(rd(p + k))) return false;
  p += k;
  return true;
}

// Rd: uint32_t operator()(uint32_t k) const, byte k of the text, called for k in [0, AC_HEAD_WIN) and
// [n - AC_TAIL_WIN, n) only.  Everything rp_match tests but the result's alphabet; sig = R | S as 16 little-endian words.
template <class Rd>
EG_FN bool ac_match_frame(const Rd& rd, uint64_t n64, accept_frame& f, uint32_t sig[16]) {
  if (n64 < RP_TEXT_MIN || n64 > RP_TEXT_MAX) return false;
  const uint32_t n = (uint32_t)n64;
  // the head, forwards
  uint32_t p = 0;
  if (!ac_lit(rd, n, p, "{\"view\":", 8)) return false;
  if (!ac_dec(rd, n, p, f.view)) return false;
  if (!ac_lit(rd, n, p, ",\"timestamp\":", 13)) return false;
  if (!ac_dec(rd, n, p, f.timestamp)) return false;
  if (!ac_lit(rd, n, p, ",\"peer_id\":\"", 12)) return false;
  f.pid_off = p;
  bool b58 = true;
  for (uint32_t i = 0; i < RP_PEER_ID_B58; ++i) b58 = b58 && ac_b58_char(rd(p + i));
  if (!b58) return false;
  p += RP_PEER_ID_B58;
  if (!ac_lit(rd, n, p, "\",\"result\":\"", 12)) return false;
  f.result_off = p;  // (at most RP_HEAD_MAX)
  // the tail, backwards: `"}` | 128 hex | `,"signature":"` | 1 .. 5 digits | `","replica":`
  uint32_t q = n - 2;
  if (rd(q) != '"' || rd(q + 1) != '}') return false;
  q -= 128;
  bool hex = true;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t w = 0; w < 16; ++w) {
    uint32_t word = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t b = 0; b < 4; ++b) {
      uint32_t hi = 0, lo = 0;
      hex = rp_m_hexval(rd(q + 8 * w + 2 * b), hi) && hex;
      hex = rp_m_hexval(rd(q + 8 * w + 2 * b + 1), lo) && hex;
      word |= ((hi << 4 | lo) & 0xFFu) << (8 * b);
    }
    sig[w] = word;
  }
  if (!hex) return false;
  q -= 14;
  {
    uint32_t t = q;
    if (!ac_lit(rd, n, t, ",\"signature\":\"", 14)) return false;
  }
  uint32_t k = 0;
  while (k < 6 && ac_digit(rd(q - 1 - k))) ++k;  // (q - 6 >= n - AC_TAIL_WIN)
  if (k == 0 || k > 5 || (k > 1 && rd(q - k) == '0')) return false;
  uint32_t rep = 0;
  for (uint32_t i = 0; i < k; ++i) rep = rep * 10 + (rd(q - k + i) - '0');
  if (rep > RP_MAX_REPLICA) return false;
  f.replica = rep;
  q -= k + 12;
  {
    uint32_t t = q;
    if (!ac_lit(rd, n, t, "\",\"replica\":", 12)) return false;
  }
  if (q < f.result_off || q - f.result_off > RP_RESULT_MAX) return false;
  f.result_len = q - f.result_off;
  return true;
}

// The signer's claim: replica < n_keys and the text's peer id is that key's (table: [n_keys][52]).
template <class Rd>
EG_FN bool ac_signer_ok(const Rd& rd, const accept_frame& f, const uint8_t* pid_table, uint32_t n_keys) {
  if (f.replica >= n_keys) return false;
  const uint8_t* want = pid_table + (size_t)RP_PEER_ID_B58 * f.replica;
  bool same = true;
  for (uint32_t i = 0; i < RP_PEER_ID_B58; ++i) same = same && rd(f.pid_off + i) == (uint32_t)want[i];
  return same;
}

// The 160-byte record as 40 words: R | S at 0, "PBFT" | 3 | view | timestamp | D at byte 64, the key index at byte 150.
EG_FN void ac_record(uint32_t rec[40], const uint32_t sig[16], uint64_t view, uint64_t timestamp, const uint32_t D[16],
                     uint32_t key) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < 16; ++j) rec[j] = sig[j];
  rec[16] = (uint32_t)'P' | (uint32_t)'B' << 8 | (uint32_t)'F' << 16 | (uint32_t)'T' << 24;
  rec[17] = RP_KIND | (uint32_t)(view << 8);
  rec[18] = (uint32_t)(view >> 24);
  rec[19] = (uint32_t)(view >> 56) | (uint32_t)(timestamp << 8);
  rec[20] = (uint32_t)(timestamp >> 24);
  uint32_t carry = (uint32_t)(timestamp >> 56);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < 16; ++j) {
    rec[21 + j] = carry | D[j] << 8;
    carry = D[j] >> 24;
  }
  rec[37] = carry | (key & 0xFFFFu) << 16;  // (byte 149 is padding)
  rec[38] = rec[39] = 0;
}
EG_FN void ac_record_none(uint32_t rec[40]) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < 40; ++j) rec[j] = 0;
  rec[37] = AC_NO_KEY << 16;
}

// Host: the whole rule for one text but the digest.  The status, and for AC_OK the head's fields and the signature.
struct ac_ptr_reader {
  const uint8_t* t;
  uint32_t operator()(uint32_t k) const { return t[k]; }
};
inline uint32_t ac_decide(const uint8_t* t, uint64_t n, const uint8_t* pid_table, uint32_t n_keys, uint32_t client,
                          uint32_t n_clients, accept_head& h, uint32_t sig[16]) {
  h = accept_head{0, 0, 0, 0, 0, AC_EDEFER};
  accept_frame f{};
  const ac_ptr_reader rd{t};
  if (!ac_match_frame(rd, n, f, sig)) return AC_EDEFER;
  if (!pr_all_alphabet(t + f.result_off, f.result_len)) return AC_EDEFER;
  if (!ac_signer_ok(rd, f, pid_table, n_keys)) return h.status = AC_ESIGNER;
  if (client >= n_clients) return h.status = AC_ECLIENT;
  h = accept_head{f.view, f.timestamp, f.result_off, f.result_len, f.replica, AC_OK};
  return AC_OK;
}

}  // namespace pbft
