// Client replies (include/pbft_wire.h pbft_sign_replies_device): the results of executed requests hashed together with
// their clients, the kind-3 envelopes signed and the canonical replies' texts written on the device, its own translation
// unit.  The text rule is reply_core.h's; the signer's state is the one pbft_sign_set_seed expanded (egress.hip), so
// every lane does the second half of RFC 8032 signing only.  The helpers are propose.hip's, copied.  Plain HIP C++.
#include "reply_kernels.h"

#include "../../include/pbft_wire.h"
#include "digest_kernels.h"
#include "verify_kernels.h"

static_assert(RP_ST_OK == PBFT_REPLY_OK && RP_ST_GENERAL == PBFT_REPLY_GENERAL && RP_RH_OK == PBFT_RH_OK &&
                  RP_RH_NONE == PBFT_RH_NONE && RP_KIND == PBFT_KIND_REPLY,
              "the core's values are the header's");
static_assert(RP_RESULT_MAX == PBFT_REPLY_RESULT_MAX && RP_PEER_ID_B58 == PBFT_REPLY_PEER_ID_CHARS, "");
static_assert(RP_MAX_N == EG_MAX_N, "the tile scan's range");

// LDS rows of one reply, in dwords; odd, so that the 64 lanes' bytewise writes at one row position fall into 64
// different banks
static constexpr uint32_t RP_ENV_DWORDS = 25;   // the 85-byte envelope, zero-padded
static constexpr uint32_t RP_HEAD_DWORDS = 35;  // RP_HEAD_MAX = 137 bytes
static constexpr uint32_t RP_TAIL_DWORDS = 41;  // RP_TAIL_MAX = 161 bytes
static_assert(4 * RP_HEAD_DWORDS >= RP_HEAD_MAX && 4 * RP_TAIL_DWORDS >= RP_TAIL_MAX && 4 * RP_ENV_DWORDS >= 96, "");
static_assert(RP_ENV_DWORDS % 2 == 1 && RP_HEAD_DWORDS % 2 == 1 && RP_TAIL_DWORDS % 2 == 1, "odd rows");

__device__ __forceinline__ uint32_t rp_wave_scan_incl(uint32_t v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}
__device__ __forceinline__ uint64_t rp_shfl64(uint64_t v, int src) {
  const uint32_t lo = __shfl((uint32_t)v, src, 64), hi = __shfl((uint32_t)(v >> 32), src, 64);
  return ((uint64_t)hi << 32) | lo;
}

// Does the result lie inside results_bytes?  (Decided before any address is formed.)
__device__ __forceinline__ bool rp_inside(uint64_t off, uint32_t len, uint64_t results_bytes) {
  return len <= results_bytes && off <= results_bytes - len;
}

// One wave per 64-reply tile.  Lane l decides about reply l from its offset and length alone; the results that are still
// candidates are then tested against the alphabet by the whole wave, 64 bytes per step with one ballot per reply (at
// most 64 * RP_RESULT_MAX / 64 steps a tile).  Then the lengths and their exclusive scan inside the tile (reply_off[i]
// holds the offset inside the tile until the signing kernel adds the tile's base); sums[t] = tile t's bytes.
__global__ void __launch_bounds__(256) reply_layout_kernel(const uint8_t* __restrict__ results, uint64_t results_bytes,
                                                           const uint64_t* __restrict__ res_off,
                                                           const uint32_t* __restrict__ res_len,
                                                           const uint64_t* __restrict__ timestamp, uint64_t view,
                                                           uint64_t N, const uint32_t* __restrict__ key,
                                                           uint64_t* __restrict__ reply_off,
                                                           uint64_t* __restrict__ sums, uint8_t* __restrict__ status) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const uint32_t replica = key[EGRESS_KEY_REPLICA];
  const bool live = i < N;
  uint64_t off = 0;
  uint32_t rl = 0;
  bool cand = false;
  if (live) {
    off = res_off[i];
    rl = res_len[i];
    cand = rp_inside(off, rl, results_bytes) && rl <= RP_RESULT_MAX;
  }
  bool res_ok = true;
  for (int r = 0; r < 64; ++r) {
    if (!__shfl((int)cand, r, 64)) continue;  // (wave-uniform)
    const uint64_t o = rp_shfl64(off, r);
    const uint32_t l = __shfl(rl, r, 64);
    bool bad = false;
    for (uint32_t k = lane; k < l; k += 64) bad = bad || !pr_alphabet(results[o + k]);
    const bool any = __ballot(bad) != 0;
    if (lane == r) res_ok = !any;
  }
  const bool ok = cand && res_ok;
  const uint32_t len = ok ? rp_text_len(view, timestamp[i], replica, rl) : 0u;
  const uint32_t incl = rp_wave_scan_incl(len, lane);
  if (live) {
    reply_off[i] = incl - len;
    status[i] = ok ? (uint8_t)RP_ST_OK : (uint8_t)RP_ST_GENERAL;
  }
  if (lane == 63 && (i - 63) < N) sums[i >> 6] = incl;
}

// One wave: sums[t] becomes the bytes in front of tile t; reply_off[N] the total.
__global__ void __launch_bounds__(64) reply_scan_kernel(uint64_t* __restrict__ sums, uint64_t n_tiles,
                                                        uint64_t* __restrict__ reply_off, uint64_t N) {
  const int lane = threadIdx.x;
  uint64_t carry = 0;
  for (uint64_t base = 0; base < n_tiles; base += 64) {
    const uint64_t t = base + lane;
    const uint32_t v = t < n_tiles ? (uint32_t)sums[t] : 0u;  // (a tile's bytes: at most 64 * RP_TEXT_MAX)
    const uint32_t incl = rp_wave_scan_incl(v, lane);
    if (t < n_tiles) sums[t] = carry + (incl - v);
    carry += __shfl(incl, 63, 64);
  }
  if (lane == 0) reply_off[N] = carry;
}

// Bytes [o, o + 4) of the string m[0, len) as a little-endian word, zero past the end, through aligned dwords of which
// at least one byte belongs to the string: for a result inside [results, results + results_bytes) with results 4-byte
// aligned, every byte read lies in [results, round_up(results_bytes, 4)).
__device__ __forceinline__ uint32_t rp_load32(const uint8_t* m, uint64_t len, uint64_t o) {
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

// D = Blake2b-512(C | m[0, len)) as 16 little-endian words: the first eight message words of block 0 are cw (the
// normalised client field), everything else comes from the result where it lies.  The hashed length is 64 + len.
__device__ __forceinline__ void rp_blake2b512(uint32_t out[16], const uint64_t cw[8], const uint8_t* m, uint64_t len) {
  uint64_t h[8] = {0x6a09e667f3bcc908ULL ^ 0x01010040ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL,
                   0xa54ff53a5f1d36f1ULL, 0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL,
                   0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
  const uint64_t total = RP_CLIENT_FIELD + len;
  const uint64_t nblocks = (total + 127) / 128;  // (at least one: total >= 64)
  for (uint64_t b = 0; b < nblocks; ++b) {
    uint64_t mw[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (b == 0 && j < 8) {
        mw[j] = cw[j];
      } else {
        const uint64_t o = 128 * b + 8 * j - RP_CLIENT_FIELD;
        mw[j] = ((uint64_t)rp_load32(m, len, o + 4) << 32) | rp_load32(m, len, o);
      }
    }
    const bool last = b == nblocks - 1;
    blake2b_compress(h, mw, last ? total : 128 * (b + 1), last);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    out[2 * i] = (uint32_t)h[i];
    out[2 * i + 1] = (uint32_t)(h[i] >> 32);
  }
}

struct rp_lds_sink {
  uint8_t* p;
  __device__ __forceinline__ void operator()(uint32_t pos, uint8_t b) const { p[pos] = b; }
};

// One wave per tile, one wave per workgroup.
//  1. Lane l hashes C | R of reply l (nothing of a result that lies outside results_bytes), builds the envelope
//     "PBFT" | 3 | view | timestamp | D in its LDS row and signs it as egress_sign_kernel does: a, prefix and A read at
//     uniform addresses, the second half of RFC 8032 signing only.  Digest and signature are stored for every reply.
//  2. A lane whose reply is canonical and ends at or below out_cap assembles the text's head and tail in its LDS rows.
//  3. The wave writes reply after reply: byte k of reply r comes from r's head row, from the result in global memory or
//     from r's tail row; the output's aligned dwords are written with one 4-byte store each (the width the proposals'
//     frame copy measured fastest), the text's unaligned ends bytewise.
__global__ void __launch_bounds__(64) reply_sign_kernel(const uint8_t* __restrict__ results, uint64_t results_bytes,
                                                        const uint64_t* __restrict__ res_off,
                                                        const uint32_t* __restrict__ res_len,
                                                        const uint64_t* __restrict__ timestamp,
                                                        const uint8_t* __restrict__ clients, uint64_t view, uint64_t N,
                                                        const uint32_t* __restrict__ key,
                                                        const uint32_t* __restrict__ tabB,
                                                        const uint64_t* __restrict__ sums,
                                                        uint64_t* __restrict__ reply_off,
                                                        const uint8_t* __restrict__ status, uint8_t* __restrict__ out,
                                                        uint64_t out_cap, uint32_t* __restrict__ digests,
                                                        uint32_t* __restrict__ sigs) {
  __shared__ __attribute__((aligned(16))) uint32_t s_env[64][RP_ENV_DWORDS];
  __shared__ __attribute__((aligned(16))) uint32_t s_head[64][RP_HEAD_DWORDS];
  __shared__ __attribute__((aligned(16))) uint32_t s_tail[64][RP_TAIL_DWORDS];
  const int lane = threadIdx.x;
  const uint64_t tile = blockIdx.x;
  const uint64_t i = tile * 64 + lane;
  const bool live = i < N;
  const uint32_t replica = key[EGRESS_KEY_REPLICA];

  uint64_t off = 0, ts = 0;
  uint32_t rl = 0;
  bool inside = false, canonical = false;
  if (live) {
    off = res_off[i];
    rl = res_len[i];
    ts = timestamp[i];
    inside = rp_inside(off, rl, results_bytes);
    canonical = status[i] == RP_ST_OK;  // (implies inside)
  }

  uint32_t dg[16], sg[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) dg[j] = sg[j] = 0;
  if (inside) {
    // C: the client field up to its first NUL, zeros behind it; every lane's field at the same stride
    const uint8_t* c = clients + (size_t)RP_CLIENT_FIELD * i;
    uint64_t cw[8];
    bool open = true;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      uint64_t w = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const uint32_t b = c[8 * j + k];
        open = open && b != 0;
        w |= (uint64_t)(open ? b : 0u) << (8 * k);
      }
      cw[j] = w;
    }
    rp_blake2b512(dg, cw, results + off, rl);
    uint8_t* e = (uint8_t*)s_env[lane];
    e[0] = 'P', e[1] = 'B', e[2] = 'F', e[3] = 'T', e[4] = (uint8_t)RP_KIND;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      e[5 + j] = (uint8_t)(view >> (8 * j));
      e[13 + j] = (uint8_t)(ts >> (8 * j));
    }
#pragma unroll
    for (int j = 0; j < 64; ++j) e[21 + j] = (uint8_t)(dg[j >> 2] >> (8 * (j & 3)));
#pragma unroll
    for (int j = PBFT_ENVELOPE_LEN; j < 4 * (int)RP_ENV_DWORDS; ++j) e[j] = 0;
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
  const uint32_t local = live ? (uint32_t)reply_off[i] : 0u;
  if (live) reply_off[i] = base + local;
  uint32_t hl = 0, tl = 0;
  if (canonical) {
    hl = rp_head_len(view, ts);
    tl = rp_tail_len(replica);
    if (base + local + hl + rl + tl <= out_cap) {  // whole replies only
      rp_lds_sink hs{(uint8_t*)s_head[lane]}, tsink{(uint8_t*)s_tail[lane]};
      rp_write_head(hs, view, ts, (const uint8_t*)(key + REPLY_KEY_PEER_ID));
      rp_write_tail(tsink, 0, replica, sg);
    } else {
      hl = tl = 0;  // no text
    }
  }
  __syncthreads();

  for (int r = 0; r < 64; ++r) {
    const uint32_t h = __shfl(hl, r, 64);
    if (h == 0) continue;  // (wave-uniform)
    const uint32_t l = __shfl(rl, r, 64), t = __shfl(tl, r, 64);
    const uint64_t o = rp_shfl64(off, r);
    const uint32_t len = h + l + t;
    uint8_t* dst = out + base + __shfl(local, r, 64);
    const uint8_t* hr = (const uint8_t*)s_head[r];
    const uint8_t* tr = (const uint8_t*)s_tail[r];
    const uint8_t* src = results + o;
    auto byte = [&](uint32_t k) -> uint32_t { return k < h ? hr[k] : (k < h + l ? src[k - h] : tr[k - h - l]); };
    uint32_t head = (uint32_t)((4 - ((uintptr_t)dst & 3)) & 3);
    if (head > len) head = len;
    const uint32_t words = (len - head) / 4;
    for (uint32_t k = lane; k < head; k += 64) dst[k] = (uint8_t)byte(k);
    for (uint32_t wd = lane; wd < words; wd += 64) {
      const uint32_t k0 = head + 4 * wd;
      *(uint32_t*)(dst + k0) = byte(k0) | byte(k0 + 1) << 8 | byte(k0 + 2) << 16 | byte(k0 + 3) << 24;
    }
    for (uint32_t k = head + 4 * words + lane; k < len; k += 64) dst[k] = (uint8_t)byte(k);
  }
}

hipError_t launch_reply(const uint8_t* d_results, uint64_t results_bytes, const uint64_t* d_res_off,
                        const uint32_t* d_res_len, const uint64_t* d_timestamp, const uint8_t* d_clients, uint64_t view,
                        uint64_t N, const uint32_t* d_key, const uint32_t* tabB, uint64_t* ws, uint8_t* d_out,
                        uint64_t out_cap, uint64_t* d_reply_off, uint8_t* d_digests, uint8_t* d_sigs, uint8_t* d_status,
                        hipStream_t st) {
  const uint64_t n_tiles = (N + REPLY_TILE - 1) / REPLY_TILE;
  if (N)
    hipLaunchKernelGGL(reply_layout_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, d_results,
                       results_bytes, d_res_off, d_res_len, d_timestamp, view, N, d_key, d_reply_off, ws, d_status);
  hipLaunchKernelGGL(reply_scan_kernel, dim3(1), dim3(64), 0, st, ws, n_tiles, d_reply_off, N);
  if (N)
    hipLaunchKernelGGL(reply_sign_kernel, dim3((unsigned)n_tiles), dim3(64), 0, st, d_results, results_bytes, d_res_off,
                       d_res_len, d_timestamp, d_clients, view, N, d_key, tabB, ws, d_reply_off, d_status, d_out,
                       out_cap, (uint32_t*)d_digests, (uint32_t*)d_sigs);
  return hipGetLastError();
}
