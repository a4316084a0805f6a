// Replica egress (include/pbft_wire.h pbft_sign_votes_frames_device): the round's own votes signed and written as
// UviBytes/JSON frames on the device, its own translation unit.  The signer's seed is expanded once
// (egress_seed_kernel); every lane of the signing kernel then does the second half of RFC 8032 signing only.
#include "egress_kernels.h"
#include "sign_tile.h"
#include "verify_kernels.h"

static constexpr uint32_t EG_ENV_DWORDS = 24;  // an envelope's LDS row: 85 bytes, zero-padded to 96
// a wave's 64 frames are contiguous in the output: at most 64 * EG_FRAME_MAX bytes, staged at the output's own
// misalignment (0..15) so that whole 16-byte granules move with one wide load and one wide store
static constexpr uint32_t EG_STAGE_BYTES = 64 * EG_FRAME_MAX + 16;
static_assert(EG_STAGE_BYTES % 16 == 0, "the staging rows stay 16-byte aligned");

__global__ void __launch_bounds__(64) egress_seed_kernel(uint32_t* __restrict__ key, uint32_t replica,
                                                         const uint32_t* __restrict__ tabB) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  uint32_t seed[8], h[16];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    seed[j] = key[EGRESS_KEY_SEED + j];
    key[EGRESS_KEY_SEED + j] = 0;
  }
  sha512_pre<32, 0>(h, seed, nullptr, 0);  // SHA-512(seed)
  uint32_t a[8], wide[16], ared[8], A[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = h[j];
  a[0] &= 0xfffffff8u;  // clamp
  a[7] &= 0x7fffffffu;
  a[7] |= 0x40000000u;
#pragma unroll
  for (int j = 0; j < 16; ++j) wide[j] = j < 8 ? a[j] : 0u;
  sc_reduce512(ared, wide);  // [a]B = [a mod L]B
  ge P;
  comb_mul_base<PLB>(P, ared, tabB);
  ge_compress_words(A, P);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    key[j] = a[j];
    key[8 + j] = h[8 + j];
    key[16 + j] = A[j];
  }
  key[EGRESS_KEY_REPLICA] = replica;
}

// Lengths, and their exclusive scan inside each 64-envelope tile (frame_off[i] holds the offset inside the tile
// until the signing kernel adds the tile's base); sums[t] = tile t's bytes.
__global__ void __launch_bounds__(256) egress_layout_kernel(const uint8_t* __restrict__ env, uint32_t stride,
                                                            uint64_t N, const uint32_t* __restrict__ key,
                                                            uint64_t* __restrict__ frame_off,
                                                            uint64_t* __restrict__ sums) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const uint32_t replica = key[EGRESS_KEY_REPLICA];
  uint32_t len = 0;
  if (i < N) {
    uint8_t head[21];
    const uint8_t* e = env + (size_t)stride * i;
#pragma unroll
    for (int j = 0; j < 21; ++j) head[j] = e[j];
    len = eg_env_frame_len(head, replica);
  }
  const uint32_t incl = wave_scan_incl(len, lane);
  if (i < N) frame_off[i] = incl - len;
  if (lane == 63 && (i - 63) < N) sums[i >> 6] = incl;
}

// One wave, for every caller of launch_tile_scan: sums[t] becomes the bytes in front of tile t; off[N] the total.
__global__ void __launch_bounds__(64) tile_scan_kernel(uint64_t* __restrict__ sums, uint64_t n_tiles,
                                                       uint64_t* __restrict__ off, uint64_t N) {
  const int lane = threadIdx.x;
  uint64_t carry = 0;
  for (uint64_t base = 0; base < n_tiles; base += 64) {
    const uint64_t t = base + lane;
    const uint32_t v = t < n_tiles ? (uint32_t)sums[t] : 0u;  // (a tile's bytes: 64 texts of a few KB each)
    const uint32_t incl = wave_scan_incl(v, lane);
    if (t < n_tiles) sums[t] = carry + (incl - v);
    carry += __shfl(incl, 63, 64);
  }
  if (lane == 0) off[N] = carry;
}

// One signature per lane, then the wave's frames.  WPB waves per workgroup; STAGED: the wave assembles its span in LDS
// and stores it with 16-byte stores (head and tail bytewise), else every lane stores its own frame bytewise.
template <int WPB, bool STAGED>
__global__ void __launch_bounds__(64 * WPB) egress_sign_kernel(const uint8_t* __restrict__ env, uint32_t stride,
                                                               uint64_t N, const uint32_t* __restrict__ key,
                                                               const uint32_t* __restrict__ tabB,
                                                               const uint64_t* __restrict__ sums,
                                                               uint64_t* __restrict__ frame_off,
                                                               uint8_t* __restrict__ out, uint64_t out_cap,
                                                               uint32_t* __restrict__ sigs) {
  __shared__ __attribute__((aligned(16))) uint32_t s_env[WPB][64][EG_ENV_DWORDS];
  __shared__ __attribute__((aligned(16))) uint8_t s_stage[STAGED ? WPB : 1][STAGED ? EG_STAGE_BYTES : 16];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint64_t wave = (uint64_t)blockIdx.x * WPB + wv;
  const uint64_t n_tiles = (N + 63) / 64;
  const uint64_t i = wave * 64 + lane;
  const bool live = i < N;
  const uint32_t replica = key[EGRESS_KEY_REPLICA];

  // the envelope, staged as zero-padded dwords: the hashes read it through aligned dwords
  uint32_t* my = s_env[wv][lane];
  const uint8_t* e = env + (size_t)stride * (live ? i : 0);
#pragma unroll
  for (int j = 0; j < (int)EG_ENV_DWORDS; ++j) {
    uint32_t w = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (4 * j + b < (int)EG_ENV_BYTES && live) w |= (uint32_t)e[4 * j + b] << (8 * b);
    my[j] = w;
  }
  const uint8_t* m = (const uint8_t*)my;
  const uint32_t kind = live ? eg_env_kind(m) : 0u;
  const uint32_t len = eg_frame_len(kind, eg_le64(m + 5), eg_le64(m + 13), replica);
  const uint64_t base = wave < n_tiles ? sums[wave] : 0;  // wave-uniform
  const uint32_t local = live ? (uint32_t)frame_off[i] : 0u;
  if (live) frame_off[i] = base + local;
  const bool fits = kind != 0 && base + local + len <= out_cap;  // whole frames only

  uint32_t R[8], S[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) R[j] = S[j] = 0;
  if (kind != 0) {
    uint32_t a[8], prefix[8], A[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {  // uniform addresses: the same words for every lane
      a[j] = key[j];
      prefix[j] = key[8 + j];
      A[j] = key[16 + j];
    }
    sign_expanded<PLB, PBFT_ENVELOPE_LEN>(R, S, a, prefix, A, m, PBFT_ENVELOPE_LEN, tabB);
  }
  if (sigs && live) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      sigs[16 * i + j] = R[j];
      sigs[16 * i + 8 + j] = S[j];
    }
  }

  if constexpr (STAGED) {
    uint8_t* dst = out + base;
    const uint32_t a0 = (uint32_t)((uintptr_t)dst & 15);
    uint8_t* stage = s_stage[wv];
    if (fits) {
      lds_sink put{stage + a0 + local};
      eg_write_frame(put, m, replica, R, S);
    }
    uint32_t span = fits ? local + len : 0u;  // the wave's bytes: the end of its last frame that fits
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = __shfl_xor(span, d, 64);
      span = o > span ? o : span;
    }
    __syncthreads();
    uint32_t head = (16 - a0) & 15;
    if (head > span) head = span;
    for (uint32_t k = lane; k < head; k += 64) dst[k] = stage[a0 + k];
    const uint32_t granules = (span - head) / 16;
    for (uint32_t k = lane; k < granules; k += 64)
      *(uint4*)(dst + head + 16 * k) = *(const uint4*)(stage + a0 + head + 16 * k);
    for (uint32_t k = head + 16 * granules + lane; k < span; k += 64) dst[k] = stage[a0 + k];
  } else {
    (void)s_stage;
    if (fits) {
      uint8_t* dst = out + base + local;
      auto put = [dst](uint32_t pos, uint8_t b) { dst[pos] = b; };
      eg_write_frame(put, m, replica, R, S);
    }
  }
}

void launch_tile_scan(uint64_t* ws, uint64_t n_tiles, uint64_t* d_off, uint64_t N, hipStream_t st) {
  hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(64), 0, st, ws, n_tiles, d_off, N);
}

hipError_t launch_egress_seed(uint32_t* d_key, uint32_t replica, const uint32_t* tabB, hipStream_t st) {
  hipLaunchKernelGGL(egress_seed_kernel, dim3(1), dim3(64), 0, st, d_key, replica, tabB);
  return hipGetLastError();
}

hipError_t launch_egress(const uint8_t* d_env, uint32_t env_stride, uint64_t N, const uint32_t* d_key,
                         const uint32_t* tabB, uint64_t* ws, uint8_t* d_out, uint64_t out_cap, uint64_t* d_frame_off,
                         uint8_t* d_sigs, int block, bool direct, hipStream_t st) {
  const uint64_t n_tiles = (N + EGRESS_TILE - 1) / EGRESS_TILE;
  if (N)
    hipLaunchKernelGGL(egress_layout_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, d_env, env_stride, N,
                       d_key, d_frame_off, ws);
  launch_tile_scan(ws, n_tiles, d_frame_off, N, st);
  if (N) {
    uint32_t* sg = (uint32_t*)d_sigs;
#define PBFT_EGRESS_LAUNCH(WPB_, ST_)                                                                              \
  hipLaunchKernelGGL((egress_sign_kernel<WPB_, ST_>), dim3((unsigned)((n_tiles + WPB_ - 1) / WPB_)), dim3(64 * WPB_), \
                     0, st, d_env, env_stride, N, d_key, tabB, ws, d_frame_off, d_out, out_cap, sg)
    if (block == 256) {
      if (direct) PBFT_EGRESS_LAUNCH(4, false);
      else PBFT_EGRESS_LAUNCH(4, true);
    } else {
      if (direct) PBFT_EGRESS_LAUNCH(1, false);
      else PBFT_EGRESS_LAUNCH(1, true);
    }
#undef PBFT_EGRESS_LAUNCH
  }
  return hipGetLastError();
}
