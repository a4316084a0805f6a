// Vote tally (include/pbft_verify.h pbft_tally_device): the verifier's bitmap, with each row's authenticated signer
// (key_idx) and envelope (env_idx), reduced on the GPU to one signer set and one distinct-signer count per envelope
// -- what Pbft::prepared / committed_local (src/behavior.rs:177-182, :214-223) ask of the message log.
// Its own translation unit; plain C++ (loads, cross-lane reads, one 8-byte atomic OR per merged group).
#include "tally_kernels.h"

// OR of v over the 64 lanes, in every lane
static __device__ __forceinline__ uint64_t wave_or(uint64_t v) {
  uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo |= (uint32_t)__shfl_xor((int)lo, o, 64);
    hi |= (uint32_t)__shfl_xor((int)hi, o, 64);
  }
  return ((uint64_t)hi << 32) | lo;
}

// One lane per row; wave w covers rows [64 w, 64 w + 64), whose valid bits are the one word bitmap[w].
// A row contributes bit (k % 64) of word e * W + k / 64 iff its bitmap bit is set, e < n_env and k < n_signers: both
// comparisons come before the word's index is formed, so no row -- whatever the bitmap says about it -- can address
// outside signers[n_env * W].
// Merge inside the wave, then one atomic per distinct word: the first still-active lane names its word, the lanes
// that share it OR their bits across the wave, that lane issues one atomicOr, and they all retire.  The replica's
// layout (a window's votes contiguous, n = 256: 64 consecutive signers of one envelope per wave) takes one turn;
// fully shuffled rows take at most 64, each a single lane's bit with no reduction.  Every order takes this loop.
__global__ void __launch_bounds__(TALLY_BLOCK) tally_kernel(const uint64_t* __restrict__ bitmap,
                                                            const uint8_t* __restrict__ key, uint32_t key_stride,
                                                            const uint8_t* __restrict__ env, uint32_t env_stride,
                                                            uint64_t N, uint32_t n_env, uint32_t n_signers, uint32_t W,
                                                            uint64_t* __restrict__ signers) {
  const uint64_t i = (uint64_t)blockIdx.x * TALLY_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63;
  if ((i & ~(uint64_t)63) >= N) return;  // the whole wave is past N (wave-uniform)
  const uint64_t valid = bitmap[i >> 6];  // uniform; word i / 64 < ceil(N / 64)
  bool active = false;
  uint64_t word = 0, bit = 0;
  if (i < N && ((valid >> lane) & 1)) {
    const uint32_t k = *(const uint16_t*)(key + i * key_stride);
    const uint32_t e = *(const uint32_t*)(env + i * env_stride);
    if (e < n_env && k < n_signers) {
      active = true;
      word = (uint64_t)e * W + (k >> 6);
      bit = (uint64_t)1 << (k & 63);
    }
  }
  uint64_t todo = __ballot(active);
  while (todo) {  // (wave-uniform: every lane takes every turn)
    const int leader = __ffsll((unsigned long long)todo) - 1;
    const uint32_t wl = __builtin_amdgcn_readlane((uint32_t)word, leader);
    const uint32_t wh = __builtin_amdgcn_readlane((uint32_t)(word >> 32), leader);
    const uint64_t w = ((uint64_t)wh << 32) | wl;
    const bool mine = active && word == w;
    const uint64_t group = __ballot(mine);
    uint64_t v = bit;  // (the leader's own bit when it is alone)
    if (group & (group - 1)) v = wave_or(mine ? bit : 0);
    if (lane == leader) atomicOr((unsigned long long*)(signers + w), (unsigned long long)v);
    active = active && !mine;
    todo &= ~group;
  }
}

// count[e] = popcount(signers[e][0..W)): G lanes per envelope (a power of two <= 64, so a group never straddles a
// wave), each summing words G apart, then a butterfly inside the group.
__global__ void __launch_bounds__(TALLY_BLOCK) tally_count_kernel(const uint64_t* __restrict__ signers, uint32_t n_env,
                                                                  uint32_t W, uint32_t G, uint32_t* __restrict__ count) {
  const uint64_t t = (uint64_t)blockIdx.x * TALLY_BLOCK + threadIdx.x;
  const uint64_t e = t / G;
  const uint32_t sub = (uint32_t)(t % G);
  int s = 0;
  if (e < n_env)
    for (uint32_t j = sub; j < W; j += G) s += __popcll((unsigned long long)signers[e * W + j]);
  for (uint32_t o = G >> 1; o > 0; o >>= 1) s += __shfl_xor(s, (int)o, 64);
  if (e < n_env && sub == 0) count[e] = (uint32_t)s;
}

// Zeroes the sets.  A kernel, not hipMemsetAsync: captured into a hipGraph between the verify and the tally, the
// memset node let the tally kernel start before the verify kernel in front of it had finished (ROCm 7, MI355X:
// replays read bitmap words the latency kernel was still writing); a chain of kernel nodes replays in order.
__global__ void __launch_bounds__(TALLY_BLOCK) tally_zero_kernel(uint64_t* __restrict__ signers, uint64_t words) {
  const uint64_t i = (uint64_t)blockIdx.x * TALLY_BLOCK + threadIdx.x;
  if (i < words) signers[i] = 0;
}

hipError_t launch_tally_zero(uint64_t* signers, uint32_t n_env, uint32_t n_signers, hipStream_t st) {
  const uint64_t words = (uint64_t)n_env * tally_words(n_signers);
  hipLaunchKernelGGL(tally_zero_kernel, dim3((unsigned)((words + TALLY_BLOCK - 1) / TALLY_BLOCK)), dim3(TALLY_BLOCK),
                     0, st, signers, words);
  return hipGetLastError();
}

hipError_t launch_tally(const uint64_t* bitmap, const uint8_t* key, uint32_t key_stride, const uint8_t* env,
                        uint32_t env_stride, uint64_t N, uint32_t n_env, uint32_t n_signers, uint64_t* signers,
                        hipStream_t st) {
  hipLaunchKernelGGL(tally_kernel, dim3((unsigned)((N + TALLY_BLOCK - 1) / TALLY_BLOCK)), dim3(TALLY_BLOCK), 0, st,
                     bitmap, key, key_stride, env, env_stride, N, n_env, n_signers, tally_words(n_signers), signers);
  return hipGetLastError();
}

hipError_t launch_tally_count(const uint64_t* signers, uint32_t n_env, uint32_t n_signers, uint32_t* count,
                              hipStream_t st) {
  const uint32_t W = tally_words(n_signers);
  uint32_t G = 1;
  while (G < W && G < 64) G <<= 1;
  const uint64_t threads = (uint64_t)n_env * G;
  hipLaunchKernelGGL(tally_count_kernel, dim3((unsigned)((threads + TALLY_BLOCK - 1) / TALLY_BLOCK)),
                     dim3(TALLY_BLOCK), 0, st, signers, n_env, W, G, count);
  return hipGetLastError();
}
