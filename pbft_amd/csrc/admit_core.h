// The replica's admission rule for one decoded frame, shared by the host (host/replica.cpp, tests/native/admit_main.cpp)
// and the device (admit.hip): from a frame's 24-byte head (pbft_frame_head of include/pbft_wire.h) and the replica's
// (view, h, log_window), what pbft_replica_push_frames would do with it before it touches a round window.
//   view first, then the window, as pbft_replica_push tests them; the window test is the replica's own in_log
//   (admit_in_log below is its one definition): seq in (h, h + log_window], written seq - h <= log_window so that a
//   window that reaches past 2^64 - 1 simply ends at 2^64 - 1 (nothing wraps).
// A vote that passes is ADMITTED; whether it is CLEAN or CONTESTED (another admitted row of the call has its (kind,
// seq, signer)) is decided over two bit planes addressed by admit_key: a row sets its bit in `seen`, and in `twice` if
// `seen` already had it, so after all rows `twice` holds exactly the keys that two or more rows share, whatever the
// order of the updates.  Every function here is the work of one lane.
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

// d_class values and d_counts indices of pbft_admit_device (PBFT_ADMIT_* of include/pbft_wire.h)
enum : uint32_t {
  ADMIT_CLEAN = 0,          // admitted vote, the only row of its (kind, seq, signer) in the call
  ADMIT_CONTESTED = 1,      // admitted vote that shares its (kind, seq, signer) with another row
  ADMIT_REJ_VIEW = 2,       // canonical vote of another view (tested before the window)
  ADMIT_REJ_WATERMARK = 3,  // canonical vote, seq outside (h, h + log_window]
  ADMIT_REJ_SIGNER = 4,     // PBFT_WIRE_ESIGNER (or a signer index >= n_keys)
  ADMIT_HOST = 5,           // any other status that is not OK, and kind 0: the host's per-frame code decides
  ADMIT_PAD = 6,            // frame number >= min(total, frame_cap)
  ADMIT_CLASSES = 8         // d_counts entries (entry 7 stays 0)
};
constexpr uint32_t ADMIT_WIRE_OK = 0, ADMIT_WIRE_ESIGNER = 5;  // PBFT_WIRE_OK, PBFT_WIRE_ESIGNER
constexpr uint64_t ADMIT_MAX_KEYS = (uint64_t)1 << 30;         // bits of one plane: 2 log_window n_keys <= 2^30

struct admit_head {  // pbft_frame_head
  uint64_t view, seq;
  uint16_t key_idx;
  uint8_t kind, status;
  uint32_t frame_len;
};

__host__ __device__ inline bool admit_in_log(uint64_t h, uint64_t log_window, uint64_t seq) {
  return seq > h && seq - h <= log_window;
}

// Bits of one plane for (log_window, n_keys), or 0 if they exceed ADMIT_MAX_KEYS (the caller then cannot use the
// planes).  log_window and n_keys are >= 1.
__host__ __device__ inline uint64_t admit_plane_bits(uint64_t log_window, uint32_t n_keys) {
  if (log_window > ADMIT_MAX_KEYS) return 0;
  const uint64_t b = 2 * log_window * (uint64_t)n_keys;  // <= 2^31 * 2^16: no overflow
  return b > ADMIT_MAX_KEYS ? 0 : b;
}

// The class of frame f but for the contest: ADMIT_CLEAN stands for "admitted".
__host__ __device__ inline uint32_t admit_classify(const admit_head& hd, uint64_t f, uint64_t n_valid, uint64_t view,
                                                   uint64_t h, uint64_t log_window, uint32_t n_keys) {
  if (f >= n_valid) return ADMIT_PAD;
  if (hd.status == ADMIT_WIRE_ESIGNER) return ADMIT_REJ_SIGNER;
  if (hd.status != ADMIT_WIRE_OK || (hd.kind != 1 && hd.kind != 2)) return ADMIT_HOST;
  if (hd.key_idx >= n_keys) return ADMIT_REJ_SIGNER;
  if (hd.view != view) return ADMIT_REJ_VIEW;
  if (!admit_in_log(h, log_window, hd.seq)) return ADMIT_REJ_WATERMARK;
  return ADMIT_CLEAN;
}

// The plane bit of an admitted row: < admit_plane_bits(log_window, n_keys), because seq - h - 1 < log_window,
// kind - 1 < 2 and key_idx < n_keys.
__host__ __device__ inline uint64_t admit_key(const admit_head& hd, uint64_t h, uint32_t n_keys) {
  return ((hd.seq - h - 1) * 2 + (uint64_t)(hd.kind - 1)) * n_keys + hd.key_idx;
}

__host__ __device__ inline bool admit_is_residue(uint32_t cls) { return cls == ADMIT_CONTESTED || cls == ADMIT_HOST; }

}  // namespace pbft
