// The primary's proposals (include/pbft_wire.h pbft_sign_preprepares_frames_device): client requests hashed, the
// PrePrepare envelopes signed and the canonical requests' frames written on the device, its own translation unit.  The
// frame rule is propose_core.h's; the signer's state is the one pbft_sign_set_seed expanded (egress.hip), so every lane
// does the second half of RFC 8032 signing only.  Plain HIP C++.
#include "propose_kernels.h"

#include "../../include/pbft_wire.h"
#include "digest_kernels.h"
#include "verify_kernels.h"
#include "wire_pp_core.h"

static_assert(PR_ST_OK == PBFT_PROPOSE_OK && PR_ST_GENERAL == PBFT_PROPOSE_GENERAL, "the core's status values are the header's");
static_assert(PR_OP_MAX == PP_OP_MAX && PR_CLIENT_MAX == PP_CLIENT_MAX && PR_BODY_MIN == PP_FRAME_MIN &&
                  PR_BODY_MAX == PP_FRAME_MAX,
              "a frame the writer emits is one the ingress matcher (wire_pp_core.h) accepts");
static_assert(PR_MAX_N == EG_MAX_N, "the tile scan's range");

// LDS rows of one request, in dwords; odd, so that the 64 lanes' bytewise writes at one row position fall into 64
// different banks
static constexpr uint32_t PR_ENV_DWORDS = 25;   // the 85-byte envelope, zero-padded
static constexpr uint32_t PR_HEAD_DWORDS = 63;  // PR_HEAD_MAX = 248 bytes
static constexpr uint32_t PR_TAIL_DWORDS = 69;  // PR_TAIL_MAX = 271 bytes
static_assert(4 * PR_HEAD_DWORDS >= PR_HEAD_MAX && 4 * PR_TAIL_DWORDS >= PR_TAIL_MAX && 4 * PR_ENV_DWORDS >= 96, "");

__device__ __forceinline__ uint32_t pr_wave_scan_incl(uint32_t v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}
__device__ __forceinline__ uint64_t pr_shfl64(uint64_t v, int src) {
  const uint32_t lo = __shfl((uint32_t)v, src, 64), hi = __shfl((uint32_t)(v >> 32), src, 64);
  return ((uint64_t)hi << 32) | lo;
}

// Does the operation lie inside ops_bytes?  (Decided before any address is formed.)
__device__ __forceinline__ bool pr_inside(uint64_t off, uint32_t len, uint64_t ops_bytes) {
  return len <= ops_bytes && off <= ops_bytes - len;
}

// One wave per 64-request tile.  Lane l decides about request l's lengths and its client; the operations of the
// requests that are still candidates are then tested against the alphabet by the whole wave, 64 bytes per step (at most
// 64 * PR_OP_MAX / 64 steps a tile).  Then the lengths and their exclusive scan inside the tile (frame_off[i] holds the
// offset inside the tile until the signing kernel adds the tile's base); sums[t] = tile t's bytes.
__global__ void __launch_bounds__(256) propose_layout_kernel(const uint8_t* __restrict__ ops, uint64_t ops_bytes,
                                                             const uint64_t* __restrict__ op_off,
                                                             const uint32_t* __restrict__ op_len,
                                                             const uint64_t* __restrict__ timestamp,
                                                             const uint8_t* __restrict__ clients, uint64_t view,
                                                             uint64_t first_seq, uint64_t N,
                                                             const uint32_t* __restrict__ key,
                                                             uint64_t* __restrict__ frame_off,
                                                             uint64_t* __restrict__ sums, uint8_t* __restrict__ status) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const uint32_t replica = key[EGRESS_KEY_REPLICA];
  const bool live = i < N;
  uint64_t off = 0;
  uint32_t ol = 0, cl = 0;
  bool cand = false;
  if (live) {
    off = op_off[i];
    ol = op_len[i];
    const uint8_t* c = clients + (size_t)PR_CLIENT_FIELD * i;
    bool c_ok = true, open = true;
    for (uint32_t k = 0; k < PR_CLIENT_FIELD; ++k) {
      const uint32_t b = c[k];
      open = open && b != 0;
      if (open) {
        ++cl;
        c_ok = c_ok && pr_alphabet(b);
      }
    }
    cand = pr_inside(off, ol, ops_bytes) && ol <= PR_OP_MAX && cl >= 1 && cl <= PR_CLIENT_MAX && c_ok;
  }
  bool op_ok = true;
  for (int r = 0; r < 64; ++r) {
    if (!__shfl((int)cand, r, 64)) continue;  // (wave-uniform)
    const uint64_t o = pr_shfl64(off, r);
    const uint32_t l = __shfl(ol, r, 64);
    bool bad = false;
    for (uint32_t k = lane; k < l; k += 64) bad = bad || !pr_alphabet(ops[o + k]);
    const bool any = __ballot(bad) != 0;
    if (lane == r) op_ok = !any;
  }
  const bool ok = cand && op_ok;
  const uint32_t len = ok ? pr_frame_len(view, first_seq + i, timestamp[i], replica, ol, cl) : 0u;
  const uint32_t incl = pr_wave_scan_incl(len, lane);
  if (live) {
    frame_off[i] = incl - len;
    status[i] = ok ? (uint8_t)PR_ST_OK : (uint8_t)PR_ST_GENERAL;
  }
  if (lane == 63 && (i - 63) < N) sums[i >> 6] = incl;
}

// One wave: sums[t] becomes the bytes in front of tile t; frame_off[N] the total.
__global__ void __launch_bounds__(64) propose_scan_kernel(uint64_t* __restrict__ sums, uint64_t n_tiles,
                                                          uint64_t* __restrict__ frame_off, uint64_t N) {
  const int lane = threadIdx.x;
  uint64_t carry = 0;
  for (uint64_t base = 0; base < n_tiles; base += 64) {
    const uint64_t t = base + lane;
    const uint32_t v = t < n_tiles ? (uint32_t)sums[t] : 0u;  // (a tile's bytes: at most 64 * PR_FRAME_MAX)
    const uint32_t incl = pr_wave_scan_incl(v, lane);
    if (t < n_tiles) sums[t] = carry + (incl - v);
    carry += __shfl(incl, 63, 64);
  }
  if (lane == 0) frame_off[N] = carry;
}

// Bytes [o, o + 4) of the string m[0, len) as a little-endian word, zero past the end, through aligned dwords of which
// at least one byte belongs to the string (the bound on what is read: propose_core.h).
__device__ __forceinline__ uint32_t pr_load32(const uint8_t* m, uint64_t len, uint64_t o) {
  if (o >= len) return 0u;
  const uintptr_t a = (uintptr_t)(m + o);
  const uint32_t* q = (const uint32_t*)(a & ~(uintptr_t)3);
  const uint32_t mis = (uint32_t)(a & 3);
  const uint32_t lo = q[0];
  const uint32_t hi = (mis && o + (4 - mis) < len) ? q[1] : 0u;
  uint32_t w = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * mis));
  const uint64_t rem = len - o;
  if (rem < 4) w &= (1u << (8 * (uint32_t)rem)) - 1u;
  return w;
}

// Blake2b-512 of m[0, len) as 16 little-endian words.
__device__ __forceinline__ void pr_blake2b512(uint32_t out[16], const uint8_t* m, uint64_t len) {
  uint64_t h[8] = {0x6a09e667f3bcc908ULL ^ 0x01010040ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL,
                   0xa54ff53a5f1d36f1ULL, 0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL,
                   0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
  const uint64_t nblocks = len == 0 ? 1 : (len + 127) / 128;
  for (uint64_t b = 0; b < nblocks; ++b) {
    uint64_t mw[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const uint64_t o = 128 * b + 8 * j;
      mw[j] = ((uint64_t)pr_load32(m, len, o + 4) << 32) | pr_load32(m, len, o);
    }
    const bool last = b == nblocks - 1;
    blake2b_compress(h, mw, last ? len : 128 * (b + 1), last);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    out[2 * i] = (uint32_t)h[i];
    out[2 * i + 1] = (uint32_t)(h[i] >> 32);
  }
}

struct pr_lds_sink {
  uint8_t* p;
  __device__ __forceinline__ void operator()(uint32_t pos, uint8_t b) const { p[pos] = b; }
};

// One wave per tile, one wave per workgroup.
//  1. Lane l hashes request l's operation where it lies (not at all if it lies outside ops_bytes), builds the envelope
//     pbft_envelope(0, view, seq, digest) in its LDS row and signs it as egress_sign_kernel does: a, prefix and A read at
//     uniform addresses, the second half of RFC 8032 signing only.  Digest and signature are stored for every request.
//  2. A lane whose request is canonical and whose frame fits below out_cap assembles the frame's head and tail in its
//     LDS rows (a wave's 64 whole frames, up to 230 KB, do not fit there).
//  3. The wave writes frame after frame: byte k of frame r comes from r's head row, from the operation in global memory
//     or from r's tail row; lane l moves the W bytes of store l, l + 64, ...  W = 1: bytewise; W = 4 / 16: the output's
//     aligned dwords / 16-byte granules with one store each, the frame's unaligned ends bytewise.
template <int W>
__global__ void __launch_bounds__(64) propose_sign_kernel(const uint8_t* __restrict__ ops, uint64_t ops_bytes,
                                                          const uint64_t* __restrict__ op_off,
                                                          const uint32_t* __restrict__ op_len,
                                                          const uint64_t* __restrict__ timestamp,
                                                          const uint8_t* __restrict__ clients, uint64_t view,
                                                          uint64_t first_seq, uint64_t N,
                                                          const uint32_t* __restrict__ key,
                                                          const uint32_t* __restrict__ tabB,
                                                          const uint64_t* __restrict__ sums,
                                                          uint64_t* __restrict__ frame_off,
                                                          const uint8_t* __restrict__ status, uint8_t* __restrict__ out,
                                                          uint64_t out_cap, uint32_t* __restrict__ digests,
                                                          uint32_t* __restrict__ sigs) {
  __shared__ __attribute__((aligned(16))) uint32_t s_env[64][PR_ENV_DWORDS];
  __shared__ __attribute__((aligned(16))) uint32_t s_head[64][PR_HEAD_DWORDS];
  __shared__ __attribute__((aligned(16))) uint32_t s_tail[64][PR_TAIL_DWORDS];
  const int lane = threadIdx.x;
  const uint64_t tile = blockIdx.x;
  const uint64_t i = tile * 64 + lane;
  const bool live = i < N;
  const uint32_t replica = key[EGRESS_KEY_REPLICA];
  const uint64_t seq = first_seq + i;

  uint64_t off = 0;
  uint32_t ol = 0;
  bool inside = false, canonical = false;
  if (live) {
    off = op_off[i];
    ol = op_len[i];
    inside = pr_inside(off, ol, ops_bytes);
    canonical = status[i] == PR_ST_OK;  // (implies inside)
  }

  uint32_t dg[16], sg[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) dg[j] = sg[j] = 0;
  if (inside) {
    pr_blake2b512(dg, ops + off, ol);
    uint8_t* e = (uint8_t*)s_env[lane];
    e[0] = 'P', e[1] = 'B', e[2] = 'F', e[3] = 'T', e[4] = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      e[5 + j] = (uint8_t)(view >> (8 * j));
      e[13 + j] = (uint8_t)(seq >> (8 * j));
    }
#pragma unroll
    for (int j = 0; j < 64; ++j) e[21 + j] = (uint8_t)(dg[j >> 2] >> (8 * (j & 3)));
#pragma unroll
    for (int j = PBFT_ENVELOPE_LEN; j < 4 * (int)PR_ENV_DWORDS; ++j) e[j] = 0;
    const uint8_t* m = e;
    uint32_t a[8], prefix[8], A[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {  // uniform addresses: the same words for every lane
      a[j] = key[j];
      prefix[j] = key[8 + j];
      A[j] = key[16 + j];
    }
    uint32_t rh[16], r[8];
    sha512_pre<32, PBFT_ENVELOPE_LEN>(rh, prefix, m, PBFT_ENVELOPE_LEN);  // r = SHA-512(prefix || M) mod L
    sc_reduce512(r, rh);
    ge P;
    comb_mul_base<PLB>(P, r, tabB);
    ge_compress_words(sg, P);
    uint32_t kh[16], k[8];
    sha512_ram<PBFT_ENVELOPE_LEN>(kh, sg, A, m, PBFT_ENVELOPE_LEN);  // k = SHA-512(R || A || M) mod L
    sc_reduce512(k, kh);
    sc_muladd(sg + 8, k, a, r);  // S = (r + k a) mod L
  }
  if (live) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      digests[16 * i + j] = dg[j];
      sigs[16 * i + j] = sg[j];
    }
  }

  const uint64_t base = sums[tile];
  const uint32_t local = live ? (uint32_t)frame_off[i] : 0u;
  if (live) frame_off[i] = base + local;
  uint32_t hl = 0, tl = 0;
  if (canonical) {
    const uint64_t ts = timestamp[i];
    const uint8_t* c = clients + (size_t)PR_CLIENT_FIELD * i;
    uint32_t cl = 0;
    while (cl < PR_CLIENT_MAX && c[cl]) ++cl;  // (canonical: a NUL within the first 64 bytes)
    hl = pr_head_len(view, seq);
    tl = pr_tail_len(ts, cl, replica);
    if (base + local + hl + ol + tl <= out_cap) {  // whole frames only
      pr_lds_sink hs{(uint8_t*)s_head[lane]}, tsink{(uint8_t*)s_tail[lane]};
      pr_write_head(hs, hl + ol + tl, view, seq, dg);
      pr_write_tail(tsink, 0, ts, c, cl, replica, sg);
    } else {
      hl = tl = 0;  // no frame
    }
  }
  __syncthreads();

  for (int r = 0; r < 64; ++r) {
    const uint32_t h = __shfl(hl, r, 64);
    if (h == 0) continue;  // (wave-uniform)
    const uint32_t l = __shfl(ol, r, 64), t = __shfl(tl, r, 64);
    const uint64_t o = pr_shfl64(off, r);
    const uint32_t len = h + l + t;
    uint8_t* dst = out + base + __shfl(local, r, 64);
    const uint8_t* hr = (const uint8_t*)s_head[r];
    const uint8_t* tr = (const uint8_t*)s_tail[r];
    const uint8_t* src = ops + o;
    auto byte = [&](uint32_t k) -> uint32_t { return k < h ? hr[k] : (k < h + l ? src[k - h] : tr[k - h - l]); };
    if constexpr (W == 1) {
      for (uint32_t k = lane; k < len; k += 64) dst[k] = (uint8_t)byte(k);
    } else {
      uint32_t head = (uint32_t)((W - ((uintptr_t)dst & (W - 1))) & (W - 1));
      if (head > len) head = len;
      const uint32_t words = (len - head) / W;
      for (uint32_t k = lane; k < head; k += 64) dst[k] = (uint8_t)byte(k);
      for (uint32_t wd = lane; wd < words; wd += 64) {
        const uint32_t k0 = head + W * wd;
        uint32_t v[W / 4];
#pragma unroll
        for (int j = 0; j < W / 4; ++j)
          v[j] = byte(k0 + 4 * j) | byte(k0 + 4 * j + 1) << 8 | byte(k0 + 4 * j + 2) << 16 | byte(k0 + 4 * j + 3) << 24;
        if constexpr (W == 4) *(uint32_t*)(dst + k0) = v[0];
        else *(uint4*)(dst + k0) = make_uint4(v[0], v[1], v[2], v[3]);
      }
      for (uint32_t k = head + W * words + lane; k < len; k += 64) dst[k] = (uint8_t)byte(k);
    }
  }
}

hipError_t launch_propose(const uint8_t* d_ops, uint64_t ops_bytes, const uint64_t* d_op_off, const uint32_t* d_op_len,
                          const uint64_t* d_timestamp, const uint8_t* d_clients, uint64_t view, uint64_t first_seq,
                          uint64_t N, const uint32_t* d_key, const uint32_t* tabB, uint64_t* ws, uint8_t* d_out,
                          uint64_t out_cap, uint64_t* d_frame_off, uint8_t* d_digests, uint8_t* d_sigs,
                          uint8_t* d_status, int width, hipStream_t st) {
  const uint64_t n_tiles = (N + PROPOSE_TILE - 1) / PROPOSE_TILE;
  if (N)
    hipLaunchKernelGGL(propose_layout_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, d_ops, ops_bytes,
                       d_op_off, d_op_len, d_timestamp, d_clients, view, first_seq, N, d_key, d_frame_off, ws, d_status);
  hipLaunchKernelGGL(propose_scan_kernel, dim3(1), dim3(64), 0, st, ws, n_tiles, d_frame_off, N);
  if (N) {
#define PBFT_PROPOSE_LAUNCH(W_)                                                                                      \
  hipLaunchKernelGGL((propose_sign_kernel<W_>), dim3((unsigned)n_tiles), dim3(64), 0, st, d_ops, ops_bytes, d_op_off, \
                     d_op_len, d_timestamp, d_clients, view, first_seq, N, d_key, tabB, ws, d_frame_off, d_status,   \
                     d_out, out_cap, (uint32_t*)d_digests, (uint32_t*)d_sigs)
    if (width == 16) PBFT_PROPOSE_LAUNCH(16);
    else if (width == 4) PBFT_PROPOSE_LAUNCH(4);
    else PBFT_PROPOSE_LAUNCH(1);
#undef PBFT_PROPOSE_LAUNCH
  }
  return hipGetLastError();
}
