// Launchers of the proposal kernels (propose.hip): N client requests -> their digests, this replica's signatures over
// the PrePrepare envelopes, and the canonical requests' signed PrePrepare frames with their offsets.  Called by
// pbft_sign_preprepares_frames_device (pbft_verify.hip), which owns the key buffer (egress_kernels.h) and the workspace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "egress_kernels.h"
#include "propose_core.h"

static constexpr uint32_t PROPOSE_TILE = 64;  // requests per scan tile: one wave
static constexpr int PROPOSE_WIDTH_DEFAULT = 4;  // bytes per store of the frame copy (PBFT_OPT_PROPOSE_WIDTH)
// the workspace of one call: one u64 per tile (its frames' bytes, then the bytes in front of it)
static inline size_t propose_ws_bytes(uint64_t N) {
  return (8 * (size_t)((N + PROPOSE_TILE - 1) / PROPOSE_TILE) + 255) & ~(size_t)255;
}

// Three kernel launches on st (the canonical test, lengths and their scan inside each tile; the scan over the tiles;
// digest, signature and frames); no allocation, copy, memset or synchronisation.  N <= PR_MAX_N; N = 0 writes
// frame_off[0] = 0 with one launch.  width: bytes per store of the frame copy, 1, 4 or 16.  ws holds
// propose_ws_bytes(N) bytes, 8-byte aligned.  d_key: the signer's state as launch_egress_seed wrote it.
hipError_t launch_propose(const uint8_t* d_ops, uint64_t ops_bytes, const uint64_t* d_op_off, const uint32_t* d_op_len,
                          const uint64_t* d_timestamp, const uint8_t* d_clients, uint64_t view, uint64_t first_seq,
                          uint64_t N, const uint32_t* d_key, const uint32_t* tabB, uint64_t* ws, uint8_t* d_out,
                          uint64_t out_cap, uint64_t* d_frame_off, uint8_t* d_digests, uint8_t* d_sigs,
                          uint8_t* d_status, int width, hipStream_t st);
