// Verification under uninstalled keys (include/pbft_verify.h pbft_verify_batch_keys): every signature carries its
// public key, and the lane computes [k](-A) itself with fixed 4-bit windows (anykey_core.h).  Its own translation unit;
// the hand-off to finish_kernel is the comb kernels'.  Plain HIP C++.
#include "anykey_kernels.h"

#include "anykey_core.h"
#include "verify_kernels.h"

// Waves per SIMD the kernel is compiled for: 3 (168 VGPRs).  Measured against 4 (128 VGPRs; the window loop then
// spills 32 registers round every addition) and 2 (256 VGPRs), each next to the table path in its own process
// (profiles/anykey/ab_waves.txt): at 2^20 signatures 3 is 4.9 % faster than 4 and 5.5 % faster than 2, at 65,536 (one
// wave per SIMD whatever the bound) the three are within the spread.
#ifndef PBFT_ANYKEY_WAVES_PER_EU
#define PBFT_ANYKEY_WAVES_PER_EU 3
#endif

// One signature per lane.  Dead lanes recompute lane 0 (no read out of bounds) and write nothing.  The lane's window
// table (anykey_core.h: 9 entries of 40 words) is a private array in scratch.
template <int LEN>
__global__ void __launch_bounds__(BLOCK, PBFT_ANYKEY_WAVES_PER_EU) anykey_kernel(
    const uint8_t* __restrict__ R, const uint8_t* __restrict__ S, const uint8_t* __restrict__ A,
    const uint8_t* __restrict__ msg, uint32_t msg_len, uint32_t msg_stride, uint64_t N,
    const uint32_t* __restrict__ tabB, uint32_t* __restrict__ xyz, uint8_t* __restrict__ flags) {
  const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  const bool live = i < N;
  const uint64_t ii = live ? i : 0;
  uint32_t r[8], s[8], a[8];
  load32(r, R + 32 * ii);
  load32(s, S + 32 * ii);
  load32(a, A + 32 * ii);
  ge P;
  const bool flag = anykey_lane<PLB, LEN>(P, r, s, a, msg + (size_t)msg_stride * ii, (int)msg_len, tabB);
  if (live) {
#pragma unroll
    for (int t = 0; t < 10; ++t) {
      xyz[(size_t)t * N + i] = P.X.v[t];
      xyz[(size_t)(10 + t) * N + i] = P.Y.v[t];
      xyz[(size_t)(20 + t) * N + i] = P.Z.v[t];
    }
    flags[i] = flag ? 1 : 0;
  }
}

hipError_t launch_anykey(const uint8_t* d_R, const uint8_t* d_S, const uint8_t* d_A, const uint8_t* d_msg,
                         uint32_t msg_len, uint32_t msg_stride, uint64_t N, const uint32_t* d_tabB, uint32_t* d_xyz,
                         uint8_t* d_flags, hipStream_t st) {
  const dim3 grid((unsigned)((N + BLOCK - 1) / BLOCK));
  if (msg_len == PBFT_ENVELOPE_LEN)
    hipLaunchKernelGGL(anykey_kernel<PBFT_ENVELOPE_LEN>, grid, dim3(BLOCK), 0, st, d_R, d_S, d_A, d_msg, msg_len,
                       msg_stride, N, d_tabB, d_xyz, d_flags);
  else
    hipLaunchKernelGGL(anykey_kernel<-1>, grid, dim3(BLOCK), 0, st, d_R, d_S, d_A, d_msg, msg_len, msg_stride, N,
                       d_tabB, d_xyz, d_flags);
  return hipGetLastError();
}

// ---- test hook: the per-lane sum on chosen scalars (pbft_debug_anykey_point) ----
// Lanes past n recompute item 0 and write nothing.  This kernel holds its own instance of anykey_sum: it tests the
// source as the device compiler sees it; the round tests check anykey_kernel as compiled.
__global__ void __launch_bounds__(64) anykey_point_kernel(const uint32_t* __restrict__ s_in,
                                                          const uint32_t* __restrict__ k_in,
                                                          const uint32_t* __restrict__ a_in, uint32_t n,
                                                          const uint32_t* __restrict__ tabB,
                                                          uint32_t* __restrict__ enc_out,
                                                          uint8_t* __restrict__ key_ok_out) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  const bool live = i < n;
  const uint32_t ii = live ? i : 0;
  uint32_t s[8], k[8], a[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) { s[t] = s_in[(size_t)8 * ii + t]; k[t] = k_in[(size_t)8 * ii + t]; a[t] = a_in[(size_t)8 * ii + t]; }
  ge P;
  bool key_ok;
  anykey_sum<PLB>(P, s, k, a, tabB, key_ok);
  uint32_t enc[8];
  ge_compress_words(enc, P);
  if (live) {
#pragma unroll
    for (int t = 0; t < 8; ++t) enc_out[(size_t)8 * i + t] = enc[t];
    key_ok_out[i] = key_ok ? 1 : 0;
  }
}

hipError_t launch_anykey_point(const uint32_t* d_s, const uint32_t* d_k, const uint32_t* d_A, uint32_t n,
                               const uint32_t* d_tabB, uint32_t* d_enc, uint8_t* d_key_ok, hipStream_t st) {
  hipLaunchKernelGGL(anykey_point_kernel, dim3((n + 63) / 64), dim3(64), 0, st, d_s, d_k, d_A, n, d_tabB, d_enc,
                     d_key_ok);
  return hipGetLastError();
}
