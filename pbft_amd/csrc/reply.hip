// Client replies (include/pbft_wire.h pbft_sign_replies_device): the results of executed requests hashed together with
// their clients, the kind-3 envelopes signed and the canonical replies' texts written on the device, its own translation
// unit.  The text rule is reply_core.h's; the signer's state is the one pbft_sign_set_seed expanded (egress.hip), so
// every lane does the second half of RFC 8032 signing only.  The wave, span, hash and copy helpers are sign_tile.h's,
// shared with propose.hip.  Plain HIP C++.
#include "reply_kernels.h"

#include "../../include/pbft_wire.h"
#include "sign_tile.h"
#include "verify_kernels.h"

static_assert(RP_ST_OK == PBFT_REPLY_OK && RP_ST_GENERAL == PBFT_REPLY_GENERAL && RP_RH_OK == PBFT_RH_OK &&
                  RP_RH_NONE == PBFT_RH_NONE && RP_KIND == PBFT_KIND_REPLY,
              "the core's values are the header's");
static_assert(RP_RESULT_MAX == PBFT_REPLY_RESULT_MAX && RP_PEER_ID_B58 == PBFT_REPLY_PEER_ID_CHARS, "");
static_assert(RP_MAX_N == EG_MAX_N, "the tile scan's range");

// LDS rows of one reply beside its envelope's (sign_tile.h), in dwords; odd, so that the 64 lanes' bytewise writes at one
// row position fall into 64 different banks
static constexpr uint32_t RP_HEAD_DWORDS = 35;  // RP_HEAD_MAX = 137 bytes
static constexpr uint32_t RP_TAIL_DWORDS = 41;  // RP_TAIL_MAX = 161 bytes
static_assert(4 * RP_HEAD_DWORDS >= RP_HEAD_MAX && 4 * RP_TAIL_DWORDS >= RP_TAIL_MAX, "");
static_assert(RP_HEAD_DWORDS % 2 == 1 && RP_TAIL_DWORDS % 2 == 1, "odd rows");

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
    cand = span_inside(off, rl, results_bytes) && rl <= RP_RESULT_MAX;
  }
  const bool res_ok = wave_span_alphabet(results, cand, off, rl, lane);
  const bool ok = cand && res_ok;
  const uint32_t len = ok ? rp_text_len(view, timestamp[i], replica, rl) : 0u;
  const uint32_t incl = wave_scan_incl(len, lane);
  if (live) {
    reply_off[i] = incl - len;
    status[i] = ok ? (uint8_t)RP_ST_OK : (uint8_t)RP_ST_GENERAL;
  }
  if (lane == 63 && (i - 63) < N) sums[i >> 6] = incl;
}

// One wave per tile, one wave per workgroup.
//  1. Lane l hashes C | R of reply l (nothing of a result that lies outside results_bytes), builds the envelope
//     "PBFT" | 3 | view | timestamp | D in its LDS row and signs it as egress_sign_kernel does: a, prefix and A read at
//     uniform addresses, the second half of RFC 8032 signing only.  Digest and signature are stored for every reply.
//  2. A lane whose reply is canonical and ends at or below out_cap assembles the text's head and tail in its LDS rows.
//  3. The wave writes reply after reply (tile_copy, sign_tile.h) with 4-byte stores, the width the proposals' frame copy
//     measured fastest.
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
  __shared__ __attribute__((aligned(16))) uint32_t s_env[64][ENV_ROW_DWORDS];
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
    inside = span_inside(off, rl, results_bytes);
    canonical = status[i] == RP_ST_OK;  // (implies inside)
  }

  uint32_t dg[16], sg[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) dg[j] = sg[j] = 0;
  if (inside) {
    uint64_t cw[8];
    client_words(cw, clients + (size_t)RP_CLIENT_FIELD * i);  // every lane's field at the same stride
    blake2b512_span<true>(dg, cw, results + off, rl);
    uint8_t* e = (uint8_t*)s_env[lane];
    envelope_row(e, RP_KIND, view, ts, dg);
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
  const uint32_t local = live ? (uint32_t)reply_off[i] : 0u;
  if (live) reply_off[i] = base + local;
  uint32_t hl = 0, tl = 0;
  if (canonical) {
    hl = rp_head_len(view, ts);
    tl = rp_tail_len(replica);
    if (base + local + hl + rl + tl <= out_cap) {  // whole replies only
      lds_sink hs{(uint8_t*)s_head[lane]}, tsink{(uint8_t*)s_tail[lane]};
      rp_write_head(hs, view, ts, (const uint8_t*)(key + REPLY_KEY_PEER_ID));
      rp_write_tail(tsink, 0, replica, sg);
    } else {
      hl = tl = 0;  // no text
    }
  }
  __syncthreads();
  tile_copy<4>(lane, hl, rl, tl, off, local, base, s_head, s_tail, results, out);
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
  launch_tile_scan(ws, n_tiles, d_reply_off, N, st);
  if (N)
    hipLaunchKernelGGL(reply_sign_kernel, dim3((unsigned)n_tiles), dim3(64), 0, st, d_results, results_bytes, d_res_off,
                       d_res_len, d_timestamp, d_clients, view, N, d_key, tabB, ws, d_reply_off, d_status, d_out,
                       out_cap, (uint32_t*)d_digests, (uint32_t*)d_sigs);
  return hipGetLastError();
}
