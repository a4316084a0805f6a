// The replica's admission pass on the device (include/pbft_wire.h pbft_admit_device): which decoded frames are votes
// the replica can apply as signer sets (clean), which go to its per-frame host code (the residue), and which are
// dropped and only counted.  The rule of one frame is admit_core.h's, the same text the host builds.
//
// Contested rows -- two or more admitted rows of one (kind, seq, signer) -- are found exactly, without hashing: an
// admitted row's seq lies in (h, h + log_window], so admit_key addresses a bit of two planes.  A row sets its bit in
// `seen` (atomicOr) and, if the bit was there already, in `twice`.  The planes only ever gain bits and `twice` ends
// with exactly the keys at least two rows share, in whatever order the atomics land; it is read after the kernel
// boundary.  Everything after that is per row or a prefix sum over one mark bit per row, as in group.hip.
// Plain C++ (loads, ballots, 4-byte atomics, 2-byte stores of the key index).  Every loop is bounded and no lane waits
// for another lane's write.
#include "admit_kernels.h"

using pbft::admit_head;

static constexpr uint32_t RECORD_BYTES = 160, RECORD_KEY = 150;  // PBFT_RECORD_BYTES, the key index's offset

static __device__ __forceinline__ uint64_t valid_frames(const uint32_t* __restrict__ n_frames, uint64_t N) {
  if (!n_frames) return N;
  const uint64_t total = n_frames[0];
  return total < N ? total : N;
}

// Both planes = 0, 16 bytes per lane, and counts[0 .. 8) = 0.  A kernel, not a memset node: see tally_zero_kernel
// (tally.hip).
__global__ void __launch_bounds__(ADMIT_BLOCK) admit_zero_kernel(uint4* __restrict__ planes, uint64_t quads,
                                                                 uint32_t* __restrict__ counts) {
  const uint64_t i = (uint64_t)blockIdx.x * ADMIT_BLOCK + threadIdx.x;
  if (i < quads) planes[i] = make_uint4(0, 0, 0, 0);
  if (i < pbft::ADMIT_CLASSES) counts[i] = 0;
}

// One lane per row: its class but for the contest, and its key's bit into the planes.
__global__ void __launch_bounds__(ADMIT_BLOCK) admit_mark_kernel(const admit_head* __restrict__ heads,
                                                                 const uint32_t* __restrict__ n_frames, uint64_t N,
                                                                 uint64_t view, uint64_t h, uint64_t log_window,
                                                                 uint32_t n_keys, uint32_t* __restrict__ seen,
                                                                 uint32_t* __restrict__ twice,
                                                                 uint8_t* __restrict__ cls) {
  const uint64_t i = (uint64_t)blockIdx.x * ADMIT_BLOCK + threadIdx.x;
  if (i >= N) return;
  const admit_head hd = heads[i];
  const uint32_t c = pbft::admit_classify(hd, i, valid_frames(n_frames, N), view, h, log_window, n_keys);
  cls[i] = (uint8_t)c;
  if (c == pbft::ADMIT_CLEAN) {
    const uint64_t k = pbft::admit_key(hd, h, n_keys);  // < admit_plane_bits(log_window, n_keys)
    const uint32_t bit = 1u << (k & 31);
    const uint32_t old = atomicOr(seen + (k >> 5), bit);
    if (old & bit) atomicOr(twice + (k >> 5), bit);
  }
}

// One lane per row, after every mark: the final class, key index 0xFFFF into the record of a row that is not clean,
// the wave's clean and residue ballot words, and the class counts (one atomic per wave and class present).
__global__ void __launch_bounds__(ADMIT_BLOCK) admit_resolve_kernel(const admit_head* __restrict__ heads, uint64_t N,
                                                                    uint64_t h, uint32_t n_keys,
                                                                    const uint32_t* __restrict__ twice,
                                                                    uint8_t* __restrict__ records,
                                                                    uint8_t* __restrict__ cls,
                                                                    uint32_t* __restrict__ counts,
                                                                    uint64_t* __restrict__ clean,
                                                                    uint64_t* __restrict__ flags) {
  const uint64_t i = (uint64_t)blockIdx.x * ADMIT_BLOCK + threadIdx.x;
  if ((i & ~(uint64_t)63) >= N) return;  // the whole wave is past N (wave-uniform)
  const bool valid = i < N;
  uint32_t c = pbft::ADMIT_CLASSES;  // (no class: a lane past N)
  if (valid) {
    c = cls[i];
    if (c == pbft::ADMIT_CLEAN) {
      const uint64_t k = pbft::admit_key(heads[i], h, n_keys);
      if ((twice[k >> 5] >> (k & 31)) & 1) {
        c = pbft::ADMIT_CONTESTED;
        cls[i] = (uint8_t)c;
      }
    }
    if (c != pbft::ADMIT_CLEAN) *(uint16_t*)(records + i * RECORD_BYTES + RECORD_KEY) = 0xFFFF;  // (an even address)
  }
  const int lane = threadIdx.x & 63;
  uint64_t m_clean = 0, m_res = 0;
#pragma unroll
  for (uint32_t q = 0; q < pbft::ADMIT_PAD + 1; ++q) {
    const uint64_t m = __ballot(valid && c == q);
    if (q == pbft::ADMIT_CLEAN) m_clean = m;
    if (pbft::admit_is_residue(q)) m_res |= m;
    if (lane == 0 && m) atomicAdd(counts + q, (uint32_t)__popcll((unsigned long long)m));
  }
  if (lane == 0) {  // word i / 64 < ceil(N / 64)
    clean[i >> 6] = m_clean;
    flags[i >> 6] = m_res;
  }
}

// prefix[w] = residue marks in words [0, w); n_res = {all marks, those beyond residue_cap}.  One block, as
// group_scan_kernel.
__global__ void __launch_bounds__(ADMIT_SCAN_BLOCK) admit_scan_kernel(const uint64_t* __restrict__ flags,
                                                                      uint64_t words, uint32_t residue_cap,
                                                                      uint32_t* __restrict__ prefix,
                                                                      uint32_t* __restrict__ n_res) {
  __shared__ uint32_t wave_sum[ADMIT_SCAN_BLOCK / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  uint32_t carry = 0;
  for (uint64_t base = 0; base < words; base += ADMIT_SCAN_BLOCK) {  // (block-uniform)
    const uint64_t idx = base + t;
    const uint32_t c = idx < words ? (uint32_t)__popcll((unsigned long long)flags[idx]) : 0;
    uint32_t v = c;  // inclusive scan inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t u = (uint32_t)__shfl_up((int)v, o, 64);
      if (lane >= o) v += u;
    }
    if (lane == 63) wave_sum[wave] = v;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < ADMIT_SCAN_BLOCK / 64; ++k) {
      const uint32_t x = wave_sum[k];
      if (k < wave) before += x;
      total += x;
    }
    if (idx < words) prefix[idx] = carry + before + v - c;
    carry += total;
    __syncthreads();
  }
  if (t == 0) {
    n_res[0] = carry;
    n_res[1] = carry > residue_cap ? carry - residue_cap : 0;
  }
}

// The residue in frame order: row i's entry number is the marks below it; entries from min(total, residue_cap) on are
// zeroed (grid-stride: residue_cap may exceed the rows).
__global__ void __launch_bounds__(ADMIT_BLOCK) admit_emit_kernel(const uint64_t* __restrict__ off,
                                                                 const uint32_t* __restrict__ len, uint64_t N,
                                                                 uint32_t residue_cap,
                                                                 const uint64_t* __restrict__ flags,
                                                                 const uint32_t* __restrict__ prefix,
                                                                 const uint32_t* __restrict__ n_res,
                                                                 admit_residue* __restrict__ res) {
  const uint64_t i = (uint64_t)blockIdx.x * ADMIT_BLOCK + threadIdx.x;
  const uint64_t threads = (uint64_t)gridDim.x * ADMIT_BLOCK;
  const uint32_t total = n_res[0];  // (the scan kernel's)
  for (uint64_t j = (uint64_t)(total < residue_cap ? total : residue_cap) + i; j < residue_cap; j += threads) {
    admit_residue z;
    z.off = 0; z.frame = 0; z.len = 0;
    res[j] = z;
  }
  if (i >= N) return;
  const uint64_t w = flags[i >> 6];
  if (!((w >> (i & 63)) & 1)) return;
  const uint32_t at = prefix[i >> 6] + (uint32_t)__popcll((unsigned long long)(w & (((uint64_t)1 << (i & 63)) - 1)));
  if (at >= residue_cap) return;
  admit_residue e;
  e.off = off ? off[i] : 0;
  e.frame = (uint32_t)i;
  e.len = len ? len[i] : 0;
  res[at] = e;
}

hipError_t launch_admit(const admit_head* heads, uint8_t* records, const uint64_t* off, const uint32_t* len,
                        const uint32_t* n_frames, uint64_t N, uint64_t view, uint64_t h, uint64_t log_window,
                        uint32_t n_keys, uint32_t residue_cap, uint8_t* ws, uint8_t* cls, uint32_t* counts,
                        uint64_t* clean, admit_residue* res, uint32_t* n_res, hipStream_t st) {
  const admit_ws L(pbft::admit_plane_bits(log_window, n_keys), N);
  uint32_t* seen = (uint32_t*)ws;
  uint32_t* twice = (uint32_t*)(ws + L.off_twice);
  uint64_t* flags = (uint64_t*)(ws + L.off_flags);
  uint32_t* prefix = (uint32_t*)(ws + L.off_prefix);
  const unsigned row_blocks = (unsigned)((N + ADMIT_BLOCK - 1) / ADMIT_BLOCK);
  const uint64_t quads = N ? L.plane_words / 2 : 0;  // (both planes: 2 plane_words / 4)
  const uint64_t zero_blocks = (quads + ADMIT_BLOCK - 1) / ADMIT_BLOCK;
  hipLaunchKernelGGL(admit_zero_kernel, dim3(zero_blocks ? (unsigned)zero_blocks : 1u), dim3(ADMIT_BLOCK), 0, st,
                     (uint4*)ws, quads, counts);
  if (N) {
    hipLaunchKernelGGL(admit_mark_kernel, dim3(row_blocks), dim3(ADMIT_BLOCK), 0, st, heads, n_frames, N, view, h,
                       log_window, n_keys, seen, twice, cls);
    hipLaunchKernelGGL(admit_resolve_kernel, dim3(row_blocks), dim3(ADMIT_BLOCK), 0, st, heads, N, h, n_keys,
                       (const uint32_t*)twice, records, cls, counts, clean, flags);
  }
  hipLaunchKernelGGL(admit_scan_kernel, dim3(1), dim3(ADMIT_SCAN_BLOCK), 0, st, (const uint64_t*)flags, L.words,
                     residue_cap, prefix, n_res);
  uint64_t res_blocks = ((uint64_t)residue_cap + ADMIT_BLOCK - 1) / ADMIT_BLOCK;
  if (res_blocks > 2048) res_blocks = 2048;
  unsigned blocks = row_blocks > (unsigned)res_blocks ? row_blocks : (unsigned)res_blocks;
  if (blocks == 0) blocks = 1;
  hipLaunchKernelGGL(admit_emit_kernel, dim3(blocks), dim3(ADMIT_BLOCK), 0, st, off, len, N, residue_cap,
                     (const uint64_t*)flags, (const uint32_t*)prefix, (const uint32_t*)n_res, res);
  return hipGetLastError();
}
