// Launchers of the vote tally (tally.hip): (bitmap, key_idx, env_idx) -> per-envelope signer sets and counts.
// Called by pbft_tally_device and by the host votes form that tallies chunk by chunk (pbft_verify.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

static constexpr int TALLY_BLOCK = 256;  // 4 waves; wave w of the grid covers rows [64 w, 64 w + 64)

// Words per envelope of the signer sets
static inline uint32_t tally_words(uint32_t n_signers) { return (n_signers + 63) / 64; }

// signers[n_env][W] = 0 (a kernel: see tally.hip for why not a memset).  n_env > 0.
hipError_t launch_tally_zero(uint64_t* signers, uint32_t n_env, uint32_t n_signers, hipStream_t st);
// ORs the N rows into signers[n_env][W] (atomics: the sets are zeroed or carry earlier pieces).  key / env are byte
// pointers to row 0's fields, read with a byte stride each.  N > 0.
hipError_t launch_tally(const uint64_t* bitmap, const uint8_t* key, uint32_t key_stride, const uint8_t* env,
                        uint32_t env_stride, uint64_t N, uint32_t n_env, uint32_t n_signers, uint64_t* signers,
                        hipStream_t st);
// count[e] = popcount of signers[e][0..W).  n_env > 0.
hipError_t launch_tally_count(const uint64_t* signers, uint32_t n_env, uint32_t n_signers, uint32_t* count,
                              hipStream_t st);
