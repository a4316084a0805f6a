// Launchers of the kernels that verify under uninstalled keys (anykey.hip; the per-lane arithmetic is anykey_core.h's).
// Called by pbft_verify_batch_keys, pbft_verify_batch_keys_device and pbft_debug_anykey_point (pbft_verify.hip), which
// own the base-point table and the workspace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// One kernel node on st: signature i = (R[i], S[i]) over msg[i][0 .. msg_len) under the key A[i] (32 raw bytes each;
// R, S, A 16-byte aligned, msg readable 16 bytes past its end) -> R' = [s]B + [k](-A) as 30 limbs in
// xyz[t * N + i] and flags[i] = s < L and the key usable: the comb kernels' hand-off, for launch_finish.  tabB: the
// base-point comb table of plan PLB.  N > 0.
hipError_t launch_anykey(const uint8_t* d_R, const uint8_t* d_S, const uint8_t* d_A, const uint8_t* d_msg,
                         uint32_t msg_len, uint32_t msg_stride, uint64_t N, const uint32_t* d_tabB, uint32_t* d_xyz,
                         uint8_t* d_flags, hipStream_t st);

// One kernel node on st: n triples (s, k, A) of 8 words each -> the encoding of [s]B + [k](-A) (8 words) and key_ok
// (one byte), through the same per-lane sum.  k < 2^253 for a meaningful point; no input reads out of bounds.
hipError_t launch_anykey_point(const uint32_t* d_s, const uint32_t* d_k, const uint32_t* d_A, uint32_t n,
                               const uint32_t* d_tabB, uint32_t* d_enc, uint8_t* d_key_ok, hipStream_t st);
