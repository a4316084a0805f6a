// Envelope grouping (include/pbft_verify.h pbft_group_envelopes_device): which rows of a batch sign the same 85-byte
// envelope.  env_idx[i] = e where envelope e is the e-th distinct envelope in row order (by first appearance, what a
// Python dict filled row by row gives), envelopes[e] its bytes, n_env their number -- the (env_idx, envelope table) pair
// pbft_tally_device and the votes forms take, made on the device from rows that are already there (the frame decoder's
// 160-byte records, or a plain column).
//
// An open-addressing table of u32 slots, a power of two >= 2 N.  A slot holds a row index -- a representative of the
// one envelope the slot stands for -- or GROUP_NONE.  A row claims an empty slot with atomicCAS; against an occupied
// one it compares its 85 bytes with the representative's, which it reads from the input: the input does not change
// during the call, so no key is ever published and no lane ever waits for another lane's write.  On a match it lowers
// the slot to its own row index (atomicMin, only when that is lower); otherwise it probes on.  A slot never changes its
// envelope and never becomes empty again, so every row of one envelope ends at the same slot, and the slot ends at
// the envelope's lowest row.  Which slot an envelope got depends on who arrived first; nothing that is written out
// does: a row's representative is the lowest row with its bytes, and an envelope's index is the number of
// representatives below its own.  That number is a prefix sum over one mark bit per row.
// Plain C++ (loads, cross-lane reads, 4-byte atomics).  Every loop is bounded and no lane spins on memory.
#include "group_kernels.h"

static constexpr int ROW_WORDS = 22;  // 21 dwords and the 85th byte

// The 85 bytes at p (any alignment) and nothing beyond them.
static __device__ __forceinline__ void load_row(const uint8_t* __restrict__ p, uint32_t w[ROW_WORDS]) {
#pragma unroll
  for (int j = 0; j < ROW_WORDS - 1; ++j) {
    uint32_t v;
    __builtin_memcpy(&v, p + 4 * j, 4);
    w[j] = v;
  }
  w[ROW_WORDS - 1] = p[84];
}

static __device__ __forceinline__ bool row_equals(const uint32_t w[ROW_WORDS], const uint8_t* __restrict__ p) {
  uint32_t o[ROW_WORDS];
  load_row(p, o);
  uint32_t diff = 0;
#pragma unroll
  for (int j = 0; j < ROW_WORDS; ++j) diff |= o[j] ^ w[j];
  return diff == 0;
}

// All 85 bytes (kind, view, seq and the whole digest among them) under the context's seed: a peer that cannot guess
// the seed cannot aim its envelopes at one probe chain.
static __device__ __forceinline__ uint64_t row_hash(const uint32_t w[ROW_WORDS], uint64_t seed) {
  uint64_t h = seed ^ 0x9E3779B97F4A7C15ull;
#pragma unroll
  for (int j = 0; j < ROW_WORDS; j += 2) {
    const uint64_t x = ((uint64_t)w[j + 1] << 32) | w[j];
    h = (h ^ x) * 0xFF51AFD7ED558CCDull;
    h ^= h >> 32;
  }
  h *= 0xC4CEB9FE1A85EC53ull;
  return h ^ (h >> 29);
}

// table[0 .. slots) = GROUP_NONE, 16 bytes per lane (slots is a multiple of 64).  A kernel, not a memset node: see
// tally_zero_kernel (tally.hip).
__global__ void __launch_bounds__(GROUP_BLOCK) group_fill_kernel(uint4* __restrict__ table, uint64_t quads) {
  const uint64_t i = (uint64_t)blockIdx.x * GROUP_BLOCK + threadIdx.x;
  if (i < quads) table[i] = make_uint4(GROUP_NONE, GROUP_NONE, GROUP_NONE, GROUP_NONE);
}

// One lane per row.  slot_of[i] = the slot of row i's envelope, GROUP_NONE for a skipped row (key index 0xFFFF).
// The wave merges first: in config #4's replica order 256 consecutive rows share an envelope, and an all-equal batch
// sends every row to one slot.  The lowest still-pending lane names its hash; lanes with that hash compare their
// bytes with its bytes (22 cross-lane reads, taken only when some other lane shares the hash) and those that match
// make it their leader.  A leader is its group's lowest lane, so its lowest row: the leaders alone go to the table,
// side by side, and hand the slot back to their group.
__global__ void __launch_bounds__(GROUP_BLOCK) group_insert_kernel(const uint8_t* __restrict__ msg, uint32_t msg_stride,
                                                                   const uint8_t* __restrict__ key,
                                                                   uint32_t key_stride, uint64_t N, uint64_t seed,
                                                                   uint64_t hash_mask, uint32_t* __restrict__ table,
                                                                   uint64_t slots, uint32_t* __restrict__ slot_of) {
  const uint64_t i = (uint64_t)blockIdx.x * GROUP_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63;
  if ((i & ~(uint64_t)63) >= N) return;  // the whole wave is past N (wave-uniform)
  bool active = i < N;
  if (active && key) active = *(const uint16_t*)(key + i * key_stride) != 0xFFFF;
  uint32_t w[ROW_WORDS];
#pragma unroll
  for (int j = 0; j < ROW_WORDS; ++j) w[j] = 0;
  uint64_t h = 0;
  if (active) {
    load_row(msg + i * msg_stride, w);
    h = row_hash(w, seed) & hash_mask;
  }
  const uint32_t h_lo = (uint32_t)h, h_hi = (uint32_t)(h >> 32);
  int leader = lane;
  bool pending = active;
  uint64_t todo = __ballot(pending);
  while (todo) {  // (wave-uniform: every lane takes every turn; the named lane retires each turn, so <= 64 turns)
    const int L = __ffsll((unsigned long long)todo) - 1;
    const uint32_t l_lo = __builtin_amdgcn_readlane(h_lo, L), l_hi = __builtin_amdgcn_readlane(h_hi, L);
    bool mine = pending && h_lo == l_lo && h_hi == l_hi;
    uint64_t group = __ballot(mine);
    if (group & (group - 1)) {  // someone shares lane L's hash: equal bytes, or a collision?
      uint32_t diff = 0;
#pragma unroll
      for (int j = 0; j < ROW_WORDS; ++j) diff |= w[j] ^ __builtin_amdgcn_readlane(w[j], L);
      mine = mine && diff == 0;
      group = __ballot(mine);
    }
    if (mine) {
      leader = L;
      pending = false;
    }
    todo &= ~group;
  }
  uint32_t slot = GROUP_NONE;
  if (active && leader == lane) {
    const uint32_t mask = (uint32_t)(slots - 1);
    uint32_t s = (uint32_t)h & mask;  // < slots
    for (uint64_t step = 0; step < slots; ++step) {
      // A look before the claim: most leaders of a frequent envelope find a lower representative and need no atomic
      // at all.  A stale value is harmless: it is empty (the CAS then tells), or an earlier row of the slot's envelope.
      uint32_t old = __hip_atomic_load(table + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (old == GROUP_NONE) old = atomicCAS(table + s, GROUP_NONE, (uint32_t)i);
      if (old == GROUP_NONE) {  // claimed
        slot = s;
        break;
      }
      if (old < N && row_equals(w, msg + (uint64_t)old * msg_stride)) {
        if (old > (uint32_t)i) atomicMin(table + s, (uint32_t)i);
        slot = s;
        break;
      }
      s = (s + 1) & mask;
    }
  }
  slot = (uint32_t)__shfl((int)slot, leader, 64);
  if (i < N) slot_of[i] = active ? slot : GROUP_NONE;
}

// flags bit i = row i is its envelope's representative (its slot holds i): one ballot word per wave.
__global__ void __launch_bounds__(GROUP_BLOCK) group_mark_kernel(const uint32_t* __restrict__ table, uint64_t slots,
                                                                 const uint32_t* __restrict__ slot_of, uint64_t N,
                                                                 uint64_t* __restrict__ flags) {
  const uint64_t i = (uint64_t)blockIdx.x * GROUP_BLOCK + threadIdx.x;
  if ((i & ~(uint64_t)63) >= N) return;
  bool rep = false;
  if (i < N) {
    const uint32_t s = slot_of[i];
    if (s < slots) rep = table[s] == (uint32_t)i;
  }
  const uint64_t m = __ballot(rep);
  if ((threadIdx.x & 63) == 0) flags[i >> 6] = m;  // word i / 64 < ceil(N / 64)
}

// prefix[w] = marks in words [0, w); n_env = {all marks, 0}.  One block: at 2^20 rows 16,384 word popcounts, 16
// tiles of 1,024.
__global__ void __launch_bounds__(GROUP_SCAN_BLOCK) group_scan_kernel(const uint64_t* __restrict__ flags,
                                                                      uint64_t words, uint32_t* __restrict__ prefix,
                                                                      uint32_t* __restrict__ n_env) {
  __shared__ uint32_t wave_sum[GROUP_SCAN_BLOCK / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  uint32_t carry = 0;
  for (uint64_t base = 0; base < words; base += GROUP_SCAN_BLOCK) {  // (block-uniform)
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
    for (int k = 0; k < GROUP_SCAN_BLOCK / 64; ++k) {
      const uint32_t x = wave_sum[k];
      if (k < wave) before += x;
      total += x;
    }
    if (idx < words) prefix[idx] = carry + before + v - c;
    carry += total;
    __syncthreads();
  }
  if (t == 0) {
    n_env[0] = carry;
    n_env[1] = 0;
  }
}

// env_idx[i] = the number of representatives below row i's own (GROUP_NONE: skipped, or that number is >= env_cap);
// each representative's wave copies its 85 bytes to envelopes[its index]; the table's entries from
// min(n_env, env_cap) on are zeroed (grid-stride: they may outnumber the rows); n_env[1] counts the rows that
// env_cap left without an index.
__global__ void __launch_bounds__(GROUP_BLOCK) group_assign_kernel(const uint8_t* __restrict__ msg, uint32_t msg_stride,
                                                                   uint64_t N, uint32_t env_cap,
                                                                   const uint32_t* __restrict__ table, uint64_t slots,
                                                                   const uint32_t* __restrict__ slot_of,
                                                                   const uint64_t* __restrict__ flags,
                                                                   const uint32_t* __restrict__ prefix,
                                                                   uint32_t* __restrict__ env_idx,
                                                                   uint8_t* __restrict__ envelopes,
                                                                   uint32_t* __restrict__ n_env) {
  const uint64_t i = (uint64_t)blockIdx.x * GROUP_BLOCK + threadIdx.x;
  const uint64_t threads = (uint64_t)gridDim.x * GROUP_BLOCK;
  const int lane = threadIdx.x & 63;
  const uint32_t found = n_env[0];  // (the scan kernel's; this kernel adds to n_env[1] only)
  const uint64_t end = (uint64_t)env_cap * GROUP_ENV_BYTES;
  for (uint64_t b = (uint64_t)(found < env_cap ? found : env_cap) * GROUP_ENV_BYTES + i; b < end; b += threads)
    envelopes[b] = 0;
  if ((i & ~(uint64_t)63) >= N) return;  // (wave-uniform)
  uint32_t rank = GROUP_NONE;
  bool is_rep = false, over = false;
  if (i < N) {
    const uint32_t s = slot_of[i];
    if (s < slots) {
      const uint32_t rep = table[s];
      if (rep < N) {
        const uint64_t below = flags[rep >> 6] & (((uint64_t)1 << (rep & 63)) - 1);
        const uint32_t r = prefix[rep >> 6] + (uint32_t)__popcll((unsigned long long)below);
        if (r < env_cap) {
          rank = r;
          is_rep = rep == (uint32_t)i;
        } else {
          over = true;
        }
      }
    }
    env_idx[i] = rank;
  }
  const uint64_t lost = __ballot(over);
  if (lane == 0 && lost) atomicAdd(n_env + 1, (uint32_t)__popcll((unsigned long long)lost));
  uint64_t reps = __ballot(is_rep);
  const uint64_t row0 = i & ~(uint64_t)63;
  while (reps) {  // (wave-uniform) lane L's row, rank < env_cap, copied by the whole wave
    const int L = __ffsll((unsigned long long)reps) - 1;
    const uint32_t r = __builtin_amdgcn_readlane(rank, L);
    const uint8_t* src = msg + (row0 + L) * msg_stride;
    uint8_t* dst = envelopes + (uint64_t)r * GROUP_ENV_BYTES;
    dst[lane] = src[lane];
    if (lane < (int)GROUP_ENV_BYTES - 64) dst[64 + lane] = src[64 + lane];
    reps &= reps - 1;
  }
}

hipError_t launch_group(const uint8_t* msg, uint32_t msg_stride, const uint8_t* key, uint32_t key_stride, uint64_t N,
                        uint32_t env_cap, uint64_t seed, uint32_t hash_bits, uint8_t* ws, uint32_t* env_idx,
                        uint8_t* envelopes, uint32_t* n_env, hipStream_t st) {
  const group_ws L(N);
  uint32_t* table = (uint32_t*)ws;
  uint32_t* slot_of = (uint32_t*)(ws + L.off_slot);
  uint64_t* flags = (uint64_t*)(ws + L.off_flags);
  uint32_t* prefix = (uint32_t*)(ws + L.off_prefix);
  const unsigned row_blocks = (unsigned)((N + GROUP_BLOCK - 1) / GROUP_BLOCK);
  if (N) {
    const uint64_t quads = L.slots / 4;
    const uint64_t hash_mask = hash_bits >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << hash_bits) - 1);
    hipLaunchKernelGGL(group_fill_kernel, dim3((unsigned)((quads + GROUP_BLOCK - 1) / GROUP_BLOCK)),
                       dim3(GROUP_BLOCK), 0, st, (uint4*)table, quads);
    hipLaunchKernelGGL(group_insert_kernel, dim3(row_blocks), dim3(GROUP_BLOCK), 0, st, msg, msg_stride, key,
                       key_stride, N, seed, hash_mask, table, L.slots, slot_of);
    hipLaunchKernelGGL(group_mark_kernel, dim3(row_blocks), dim3(GROUP_BLOCK), 0, st, (const uint32_t*)table, L.slots,
                       (const uint32_t*)slot_of, N, flags);
  }
  hipLaunchKernelGGL(group_scan_kernel, dim3(1), dim3(GROUP_SCAN_BLOCK), 0, st, (const uint64_t*)flags, L.words,
                     prefix, n_env);
  // enough blocks for the rows, and for a table much larger than the batch a share of its zero-fill
  uint64_t zero_blocks = ((uint64_t)env_cap * GROUP_ENV_BYTES + 16 * GROUP_BLOCK - 1) / (16 * GROUP_BLOCK);
  if (zero_blocks > 2048) zero_blocks = 2048;
  unsigned blocks = row_blocks > (unsigned)zero_blocks ? row_blocks : (unsigned)zero_blocks;
  if (blocks == 0) blocks = 1;
  hipLaunchKernelGGL(group_assign_kernel, dim3(blocks), dim3(GROUP_BLOCK), 0, st, msg, msg_stride, N, env_cap,
                     (const uint32_t*)table, L.slots, (const uint32_t*)slot_of, (const uint64_t*)flags,
                     (const uint32_t*)prefix, env_idx, envelopes, n_env);
  return hipGetLastError();
}
