// The pure-host half of the blocking signing forms (pbft_sign_votes_frames, pbft_sign_preprepares_frames,
// pbft_sign_replies in pbft_verify.hip): where each region of the shared device staging lies, whether every item lies
// inside its payload, and how the device's packed bytes and the host encoder's general items become one stream.  No HIP
// call and no device code: a CPU program includes this header and runs it under sanitizers
// (tests/native/sign_host_main.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "egress_core.h"  // EG_ENV_BYTES

namespace pbft {

// Device staging of one blocking call, every region rounded up to 256 bytes:
//   payload (+ 16: the kernels read whole 16-byte words) | offsets | lengths | timestamps | clients | output offsets
//   | digests | signatures | status | the bytes the device writes
// for N items over a payload of payload_bytes.  The votes form has envelopes for a payload and neither per-item inputs
// nor digests nor status: those regions are empty and its layout is envelopes | frame_off | sigs | frames.
struct sign_layout {
  size_t off, len, ts, cl, out_off, dig, sig, st, out, total;  // (the payload is at 0)
  static size_t up(size_t b) { return (b + 255) & ~(size_t)255; }
  sign_layout(uint64_t N, size_t payload_bytes, size_t dev_bytes, bool items = true) {
    const size_t n = (size_t)N, k = items ? n : 0;
    off = up(payload_bytes + (items ? 16 : 0));
    len = off + up(8 * k);
    ts = len + up(4 * k);
    cl = ts + up(8 * k);
    out_off = cl + up(64 * k);
    dig = out_off + up(8 * (n + 1));
    sig = dig + up(64 * k);
    st = sig + up(64 * n);
    out = st + up(k);
    total = out + up(dev_bytes);
  }
};

// The envelopes of the votes form: N rows env_stride apart, the last one not padded (N >= 1).
inline size_t sign_votes_env_bytes(uint32_t env_stride, uint64_t N) {
  return (size_t)env_stride * (size_t)(N - 1) + EG_ENV_BYTES;
}
inline sign_layout sign_votes_layout(uint32_t env_stride, uint64_t N, size_t dev_bytes) {
  return sign_layout(N, sign_votes_env_bytes(env_stride, N), dev_bytes, false);
}

// Every item [off[i], off[i] + len[i]) lies inside [0, bytes); no sum that could wrap.
inline bool sign_spans_inside(const uint64_t* off, const uint32_t* len, uint64_t N, uint64_t bytes) {
  for (uint64_t i = 0; i < N; ++i)
    if (len[i] > bytes || off[i] > bytes - len[i]) return false;
  return true;
}

// What the host's dry run says the device will write: the items of status dev_status, packed in order.
struct sign_split {
  uint64_t n_general = 0;
  size_t dev_bytes = 0;
};
inline sign_split sign_count(const uint64_t* h_off, const uint8_t* h_st, uint64_t N, uint8_t dev_status) {
  sign_split s;
  for (uint64_t i = 0; i < N; ++i) {
    if (h_st[i] == dev_status) s.dev_bytes += (size_t)(h_off[i + 1] - h_off[i]);
    else ++s.n_general;
  }
  return s;
}

// The complete stream, on the host: item i occupies out + [h_off[i], h_off[i + 1]).  The device's items (status
// dev_status) are copied in order from its packed bytes `dev`; every other one is written by
// encode(i, out + h_off[i], its length, &got), which returns nonzero on an error.  False: an encode failed or wrote
// another length than the dry run said.
template <class Encode>
inline bool sign_merge(uint64_t N, const uint64_t* h_off, const uint8_t* h_st, uint8_t dev_status, const uint8_t* dev,
                       uint8_t* out, Encode&& encode) {
  size_t from = 0;
  for (uint64_t i = 0; i < N; ++i) {
    const size_t at = (size_t)h_off[i], fl = (size_t)(h_off[i + 1] - h_off[i]);
    if (h_st[i] == dev_status) {
      if (fl) memcpy(out + at, dev + from, fl);
      from += fl;
      continue;
    }
    size_t got = 0;
    if (encode(i, out + at, fl, &got) || got != fl) return false;
  }
  return true;
}

}  // namespace pbft
