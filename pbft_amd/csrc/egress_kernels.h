// Launchers of the egress kernels (egress.hip): N 85-byte envelopes -> this replica's signed vote frames, their
// offsets and (optionally) the signatures.  Called by pbft_sign_set_seed / pbft_sign_votes_frames_device
// (pbft_verify.hip), which own the key buffer and the workspace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "egress_core.h"

// The signer's state on the device: a (clamped) | prefix | A as 24 little-endian words, the replica index at word
// EGRESS_KEY_REPLICA; the seed is staged at word EGRESS_KEY_SEED for the expansion kernel, which zeroes it.
static constexpr uint32_t EGRESS_KEY_REPLICA = 24, EGRESS_KEY_SEED = 32, EGRESS_KEY_WORDS = 64;
static constexpr uint32_t EGRESS_TILE = 64;  // envelopes per scan tile: one wave
// the workspace of one call: one u64 per tile (its frames' bytes, then the bytes in front of it)
static inline size_t egress_ws_bytes(uint64_t N) {
  return (8 * (size_t)((N + EGRESS_TILE - 1) / EGRESS_TILE) + 255) & ~(size_t)255;
}

// One lane: SHA-512(seed) -> a, prefix; A = [a]B; key[0..24) and key[EGRESS_KEY_REPLICA] written, the seed zeroed.
hipError_t launch_egress_seed(uint32_t* d_key, uint32_t replica, const uint32_t* tabB, hipStream_t st);

// The scan over the tiles, for the egress, proposal and reply launchers alike (one wave, one launch on st): ws[t], tile
// t's bytes, becomes the bytes in front of tile t, and d_off[N] the total.  n_tiles <= EG_MAX_N / EGRESS_TILE; a failed launch shows in the caller's hipGetLastError.
void launch_tile_scan(uint64_t* ws, uint64_t n_tiles, uint64_t* d_off, uint64_t N, hipStream_t st);

// Three kernel launches on st (lengths and their scan inside each tile, the scan over the tiles, sign and write); no
// allocation, copy, memset or synchronisation.  N <= EG_MAX_N; N = 0 writes frame_off[0] = 0 with one launch.
// block: 64 or 256 lanes per workgroup of the signing kernel; direct: every lane stores its own frame bytewise
// instead of the wave staging its span in LDS.  ws holds egress_ws_bytes(N) bytes, 8-byte aligned.
hipError_t launch_egress(const uint8_t* d_env, uint32_t env_stride, uint64_t N, const uint32_t* d_key,
                         const uint32_t* tabB, uint64_t* ws, uint8_t* d_out, uint64_t out_cap, uint64_t* d_frame_off,
                         uint8_t* d_sigs, int block, bool direct, hipStream_t st);
