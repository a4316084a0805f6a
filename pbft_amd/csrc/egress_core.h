// The canonical signed vote frame written from its 85-byte envelope, shared by the host (length queries of
// pbft_sign_votes_frames and pbft_replica_emit_frames) and the device (egress.hip):
//   varint(len) {"Prepare":{"view":V,"sequence_number":N,"digest":"<128 hex>","replica":R,"signature":"<128 hex>"}}
// (or "Commit"), byte for byte what pbft_wire_encode_votes writes (host/wire.cpp).  The envelope is
// "PBFT" | kind | view LE | seq LE | digest[64] (pbft_envelope): everything of the frame but the signer's index and
// the signature.  A frame's length depends only on the kind and on the decimal widths of view, seq and replica; the
// body is EG_BODY_MIN .. EG_BODY_MAX bytes (PBFT_FRAME_MIN .. PBFT_FRAME_MAX), so its varint always has two bytes.
// An envelope whose magic is wrong or whose kind is not 1 or 2 has no frame: length 0.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define EG_FN __host__ __device__ __forceinline__
#else
#define EG_FN inline
#endif

namespace pbft {

constexpr uint32_t EG_ENV_BYTES = 85;
constexpr uint32_t EG_MAX_REPLICA = 65535;  // at most five digits: the bound of EG_FRAME_MAX
constexpr uint64_t EG_MAX_N = (uint64_t)1 << 24;

#define PBFT_EG_L0P "{\"Prepare\":{\"view\":"
#define PBFT_EG_L0C "{\"Commit\":{\"view\":"
#define PBFT_EG_L1 ",\"sequence_number\":"
#define PBFT_EG_L2 ",\"digest\":\""
#define PBFT_EG_L3 "\",\"replica\":"
#define PBFT_EG_L4 ",\"signature\":\""
#define PBFT_EG_L5 "\"}}"
constexpr uint32_t EG_SKELETON = (uint32_t)(sizeof(PBFT_EG_L1 PBFT_EG_L2 PBFT_EG_L3 PBFT_EG_L4 PBFT_EG_L5) - 1) + 2 * 128;
constexpr uint32_t EG_BODY_MIN = EG_SKELETON + (uint32_t)sizeof(PBFT_EG_L0C) - 1 + 3;
constexpr uint32_t EG_BODY_MAX = EG_SKELETON + (uint32_t)sizeof(PBFT_EG_L0P) - 1 + 20 + 20 + 5;
constexpr uint32_t EG_FRAME_MAX = EG_BODY_MAX + 2;  // with the two-byte varint
static_assert(EG_BODY_MIN == 336 && EG_BODY_MAX == 379, "the vote frame's length window (PBFT_FRAME_MIN / _MAX)");
static_assert(EG_BODY_MIN >= 128 && EG_BODY_MAX < 16384, "a two-byte varint");

EG_FN uint32_t eg_dec_width(uint64_t v) {
  uint32_t w = 1;
  while (v >= 10) {
    v /= 10;
    ++w;
  }
  return w;
}

EG_FN uint64_t eg_le64(const uint8_t* p) {
  uint64_t v = 0;
  for (int i = 7; i >= 0; --i) v = (v << 8) | p[i];
  return v;
}

// The kind of a well-formed envelope (1 Prepare, 2 Commit), 0 of any other.
EG_FN uint32_t eg_env_kind(const uint8_t* env) {
  if (env[0] != 'P' || env[1] != 'B' || env[2] != 'F' || env[3] != 'T') return 0;
  return (env[4] == 1 || env[4] == 2) ? env[4] : 0;
}

// Bytes of the frame (varint included) of a vote of `kind` (1 / 2); 0 for kind 0.
EG_FN uint32_t eg_frame_len(uint32_t kind, uint64_t view, uint64_t seq, uint32_t replica) {
  if (kind == 0) return 0;
  const uint32_t l0 = kind == 1 ? (uint32_t)sizeof(PBFT_EG_L0P) - 1 : (uint32_t)sizeof(PBFT_EG_L0C) - 1;
  return 2 + EG_SKELETON + l0 + eg_dec_width(view) + eg_dec_width(seq) + eg_dec_width(replica);
}
EG_FN uint32_t eg_env_frame_len(const uint8_t* env, uint32_t replica) {
  return eg_frame_len(eg_env_kind(env), eg_le64(env + 5), eg_le64(env + 13), replica);
}

// Sink: void operator()(uint32_t pos, uint8_t byte), pos relative to the frame's first byte.
template <class Sink>
EG_FN uint32_t eg_put_lit(Sink& put, uint32_t pos, const char* s, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) put(pos + i, (uint8_t)s[i]);
  return pos + n;
}
template <class Sink>
EG_FN uint32_t eg_put_dec(Sink& put, uint32_t pos, uint64_t v) {
  const uint32_t w = eg_dec_width(v);
  for (uint32_t i = w; i-- > 0;) {
    put(pos + i, (uint8_t)('0' + (uint32_t)(v % 10)));
    v /= 10;
  }
  return pos + w;
}
EG_FN uint8_t eg_hex(uint32_t nib) { return (uint8_t)(nib < 10 ? '0' + nib : 'a' + (nib - 10)); }
// 4 * n_words bytes given as little-endian words -> 8 * n_words lowercase hex digits
template <class Sink>
EG_FN uint32_t eg_put_hex_words(Sink& put, uint32_t pos, const uint32_t* w, int n_words) {
  for (int j = 0; j < n_words; ++j)
    for (int b = 0; b < 4; ++b) {
      const uint32_t v = (w[j] >> (8 * b)) & 0xFF;
      put(pos + 8 * j + 2 * b, eg_hex(v >> 4));
      put(pos + 8 * j + 2 * b + 1, eg_hex(v & 15));
    }
  return pos + 8 * n_words;
}
template <class Sink>
EG_FN uint32_t eg_put_hex_bytes(Sink& put, uint32_t pos, const uint8_t* p, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) {
    put(pos + 2 * i, eg_hex(p[i] >> 4));
    put(pos + 2 * i + 1, eg_hex(p[i] & 15));
  }
  return pos + 2 * n;
}

// The whole frame of a well-formed envelope (kind 1 / 2) signed by `replica` with R, S (8 LE words each); returns
// its length, eg_frame_len of the same fields.
template <class Sink>
EG_FN uint32_t eg_write_frame(Sink& put, const uint8_t* env, uint32_t replica, const uint32_t R[8], const uint32_t S[8]) {
  const uint32_t kind = env[4];
  const uint64_t view = eg_le64(env + 5), seq = eg_le64(env + 13);
  const uint32_t body = eg_frame_len(kind, view, seq, replica) - 2;
  put(0, (uint8_t)(0x80 | (body & 0x7F)));
  put(1, (uint8_t)(body >> 7));
  uint32_t p = 2;
  if (kind == 1) p = eg_put_lit(put, p, PBFT_EG_L0P, (uint32_t)sizeof(PBFT_EG_L0P) - 1);
  else p = eg_put_lit(put, p, PBFT_EG_L0C, (uint32_t)sizeof(PBFT_EG_L0C) - 1);
  p = eg_put_dec(put, p, view);
  p = eg_put_lit(put, p, PBFT_EG_L1, (uint32_t)sizeof(PBFT_EG_L1) - 1);
  p = eg_put_dec(put, p, seq);
  p = eg_put_lit(put, p, PBFT_EG_L2, (uint32_t)sizeof(PBFT_EG_L2) - 1);
  p = eg_put_hex_bytes(put, p, env + 21, 64);
  p = eg_put_lit(put, p, PBFT_EG_L3, (uint32_t)sizeof(PBFT_EG_L3) - 1);
  p = eg_put_dec(put, p, replica);
  p = eg_put_lit(put, p, PBFT_EG_L4, (uint32_t)sizeof(PBFT_EG_L4) - 1);
  p = eg_put_hex_words(put, p, R, 8);
  p = eg_put_hex_words(put, p, S, 8);
  p = eg_put_lit(put, p, PBFT_EG_L5, (uint32_t)sizeof(PBFT_EG_L5) - 1);
  return p;
}

}  // namespace pbft
