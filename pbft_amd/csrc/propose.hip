// The primary's proposals (include/pbft_wire.h pbft_sign_preprepares_frames_device): client requests hashed, the
// PrePrepare envelopes signed and the canonical requests' frames written on the device, its own translation unit.  The
// frame rule is propose_core.h's; the signer's state is the one pbft_sign_set_seed expanded (egress.hip), so every lane
// does the second half of RFC 8032 signing only.  Plain HIP C++.
#include "propose_kernels.h"

#include "../../include/pbft_wire.h"
#include "sign_tile.h"
#include "verify_kernels.h"
#include "wire_pp_core.h"

static_assert(PR_ST_OK == PBFT_PROPOSE_OK && PR_ST_GENERAL == PBFT_PROPOSE_GENERAL, "the core's status values are the header's");
static_assert(PR_OP_MAX == PP_OP_MAX && PR_CLIENT_MAX == PP_CLIENT_MAX && PR_BODY_MIN == PP_FRAME_MIN &&
                  PR_BODY_MAX == PP_FRAME_MAX,
              "a frame the writer emits is one the ingress matcher (wire_pp_core.h) accepts");
static_assert(PR_MAX_N == EG_MAX_N, "the tile scan's range");

// LDS rows of one request beside its envelope's (sign_tile.h), in dwords; odd, so that the 64 lanes' bytewise writes at
// one row position fall into 64 different banks
static constexpr uint32_t PR_HEAD_DWORDS = 63;  // PR_HEAD_MAX = 248 bytes
static constexpr uint32_t PR_TAIL_DWORDS = 69;  // PR_TAIL_MAX = 271 bytes
static_assert(4 * PR_HEAD_DWORDS >= PR_HEAD_MAX && 4 * PR_TAIL_DWORDS >= PR_TAIL_MAX, "");

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
    cand = span_inside(off, ol, ops_bytes) && ol <= PR_OP_MAX && cl >= 1 && cl <= PR_CLIENT_MAX && c_ok;
  }
  const bool op_ok = wave_span_alphabet(ops, cand, off, ol, lane);
  const bool ok = cand && op_ok;
  const uint32_t len = ok ? pr_frame_len(view, first_seq + i, timestamp[i], replica, ol, cl) : 0u;
  const uint32_t incl = wave_scan_incl(len, lane);
  if (live) {
    frame_off[i] = incl - len;
    status[i] = ok ? (uint8_t)PR_ST_OK : (uint8_t)PR_ST_GENERAL;
  }
  if (lane == 63 && (i - 63) < N) sums[i >> 6] = incl;
}

// One wave per tile, one wave per workgroup.
//  1. Lane l hashes request l's operation where it lies (not at all if it lies outside ops_bytes), builds the envelope
//     pbft_envelope(0, view, seq, digest) in its LDS row and signs it as egress_sign_kernel does: a, prefix and A read at
//     uniform addresses, the second half of RFC 8032 signing only.  Digest and signature are stored for every request.
//  2. A lane whose request is canonical and whose frame fits below out_cap assembles the frame's head and tail in its
//     LDS rows (a wave's 64 whole frames, up to 230 KB, do not fit there).
//  3. The wave writes frame after frame (tile_copy, sign_tile.h) with stores of W bytes: 1, 4 or 16.
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
  __shared__ __attribute__((aligned(16))) uint32_t s_env[64][ENV_ROW_DWORDS];
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
    inside = span_inside(off, ol, ops_bytes);
    canonical = status[i] == PR_ST_OK;  // (implies inside)
  }

  uint32_t dg[16], sg[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) dg[j] = sg[j] = 0;
  if (inside) {
    blake2b512_span<false>(dg, nullptr, ops + off, ol);
    uint8_t* e = (uint8_t*)s_env[lane];
    envelope_row(e, 0, view, seq, dg);
    uint32_t a[8], prefix[8], A[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {  // uniform addresses: the same words for every lane
      a[j] = key[j];
      prefix[j] = key[8 + j];
      A[j] = key[16 + j];
    }
    sign_expanded<PLB, PBFT_ENVELOPE_LEN>(sg, sg + 8, a, prefix, A, e, PBFT_ENVELOPE_LEN, tabB);
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
      lds_sink hs{(uint8_t*)s_head[lane]}, tsink{(uint8_t*)s_tail[lane]};
      pr_write_head(hs, hl + ol + tl, view, seq, dg);
      pr_write_tail(tsink, 0, ts, c, cl, replica, sg);
    } else {
      hl = tl = 0;  // no frame
    }
  }
  __syncthreads();
  tile_copy<W>(lane, hl, ol, tl, off, local, base, s_head, s_tail, ops, out);
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
  launch_tile_scan(ws, n_tiles, d_frame_off, N, st);
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
