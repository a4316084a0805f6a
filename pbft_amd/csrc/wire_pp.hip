// PrePrepares of the admission pass's residue, parsed and digested on the GPU (include/pbft_wire.h
// pbft_wire_decode_preprepares_device), and the host build of the same rule (pbft_wire_decode_preprepare).
// The rule is wire_pp_core.h's.  Its own translation unit; plain C++ (16-byte loads, LDS, ballots, 8-byte stores).
#include "wire_pp_kernels.h"

#include <string.h>

#include "../../include/pbft_wire.h"
#include "wire_pp_core.h"

using namespace pbft;

static_assert(PP_ST_NONE == PBFT_PP_NONE && PP_ST_OK == PBFT_PP_OK, "the core's status values are the header's");
static_assert(PP_OP_MAX == PBFT_PP_OP_MAX && PP_FRAME_MIN == PBFT_PP_FRAME_MIN && PP_FRAME_MAX == PBFT_PP_FRAME_MAX,
              "the core's limits are the header's");
static_assert(sizeof(pbft_pp_head) == 232 && offsetof(pbft_pp_head, op_off) == 24 &&
                  offsetof(pbft_pp_head, replica) == 32 && offsetof(pbft_pp_head, status) == 34 &&
                  offsetof(pbft_pp_head, claimed) == 40 && offsetof(pbft_pp_head, computed) == 104 &&
                  offsetof(pbft_pp_head, sig) == 168,
              "29 8-byte stores per head");
static_assert(sizeof(pbft_admit_residue) == 16, "one 16-byte load per entry");
static_assert(sizeof(uint4) * PP_ROW_GRANULES < 4096, "a wave's row stays under 4 KB of LDS");

static constexpr uint32_t HEAD_WORDS = sizeof(pbft_pp_head) / 8;

struct pp_lds_row {
  const uint32_t* row;
  __device__ __forceinline__ uint32_t dword(uint32_t i) const { return row[i]; }
};

// The scanner of the two free strings over the whole wave: per step lane l classes the four bytes of dword l of a
// 256-byte window, a ballot finds the first lane with a byte outside the alphabet, a shuffle fetches which byte it is.
// At most ceil((PP_OP_MAX + 4) / 256) + 1 steps.  Called by all 64 lanes in step.
struct pp_wave_scan {
  const uint32_t* row;
  uint32_t lane;
  __device__ __forceinline__ uint32_t operator()(uint32_t from, uint32_t limit) const {
    for (uint32_t base = from & ~3u; base < limit; base += 256) {
      const uint32_t at = base + 4 * lane;
      uint32_t first = 4;
      if (at < limit) {
        const uint32_t w = row[at >> 2];
#pragma unroll
        for (int b = 3; b >= 0; --b) {
          const uint32_t pos = at + b;
          if (pos >= from && pos < limit && !pp_alphabet((w >> (8 * b)) & 0xFFu)) first = b;
        }
      }
      const unsigned long long m = __ballot(first < 4);
      if (m) {
        const int f = __ffsll(m) - 1;
        return base + 4 * f + __shfl(first, f);
      }
    }
    return limit;
  }
};

// One wave per residue entry, one wave per block.
//  1. The entry's bounds, before any address is formed: PP_FRAME_MIN <= len <= PP_FRAME_MAX and off + len <=
//     stream_bytes.  An entry that fails -- every vote of the residue does, by its length -- is PBFT_PP_NONE and none
//     of its bytes are read; so is an entry at or behind the live count.
//  2. The wave stages the frame into LDS: lane l loads the 16-byte granules l, l + 64, ... of the span that holds the
//     frame, all inside [d_stream, d_stream + round_up(stream_bytes, 16)), so the frame starts at byte off % 16 of
//     the row.
//  3. All 64 lanes run wire_pp_frame over the row in step.  Every LDS read of the skeleton and the numbers is one
//     address for the whole wave (a broadcast), so this costs what lane 0 alone would cost, and the two free strings
//     can use every lane without handing a cursor from lane 0 to the wave and back.  A frame that is not a PrePrepare
//     leaves at the first literal.
//  4. Lane 0 writes the head, `computed` zero: pp_digest_kernel fills it in.
__global__ void __launch_bounds__(64) pp_parse_kernel(const uint8_t* __restrict__ stream, uint64_t stream_bytes,
                                                      const pbft_admit_residue* __restrict__ res,
                                                      const uint32_t* __restrict__ n_res, uint32_t n_entries,
                                                      uint2* __restrict__ pp) {
  __shared__ uint4 row[PP_ROW_GRANULES];
  const uint32_t i = blockIdx.x, lane = threadIdx.x;
  uint32_t live = n_entries;
  if (n_res) live = n_res[0] < n_entries ? n_res[0] : n_entries;
  uint32_t n = 0;  // the length if the frame may be read, else 0
  uint64_t off = 0;
  if (i < live) {
    const pbft_admit_residue e = res[i];
    if (e.len >= PP_FRAME_MIN && e.len <= PP_FRAME_MAX && stream_bytes >= e.len && e.off <= stream_bytes - e.len) {
      n = e.len;
      off = e.off;
    }
  }
  const uint32_t a = (uint32_t)off & 15u;
  if (n) {  // (wave-uniform)
    const uint32_t G = (a + n + 15) / 16;  // <= PP_ROW_GRANULES - 1
    const uint4* src = (const uint4*)(stream + (off - a));
    for (uint32_t g = lane; g < G; g += 64) row[g] = src[g];
    __syncthreads();
  }
  pp_fields h;
  wire_pp_frame(pp_lds_row{(const uint32_t*)row}, pp_wave_scan{(const uint32_t*)row, lane}, a, n, h);
  if (lane != 0) return;
  uint2* out = pp + (uint64_t)i * HEAD_WORDS;
  out[0] = make_uint2((uint32_t)h.view, (uint32_t)(h.view >> 32));
  out[1] = make_uint2((uint32_t)h.seq, (uint32_t)(h.seq >> 32));
  out[2] = make_uint2((uint32_t)h.timestamp, (uint32_t)(h.timestamp >> 32));
  out[3] = make_uint2(h.op_off, h.op_len);
  out[4] = make_uint2(h.replica | (h.status << 16), 0);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    out[5 + k] = make_uint2(h.claimed[2 * k], h.claimed[2 * k + 1]);
    out[13 + k] = make_uint2(0, 0);
    out[21 + k] = make_uint2(h.sig[2 * k], h.sig[2 * k + 1]);
  }
}

// One lane per entry, as digest_kernel<0>: a lane whose head is PBFT_PP_OK hashes the operation where it lies in the
// stream (what is read: wire_pp_core.h) and stores `computed`.  Lanes differ only in the number of 128-byte blocks.
__global__ void __launch_bounds__(64) pp_digest_kernel(const uint8_t* __restrict__ stream,
                                                       const pbft_admit_residue* __restrict__ res, uint32_t n_entries,
                                                       uint2* __restrict__ pp) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n_entries) return;
  uint2* hd = pp + (uint64_t)i * HEAD_WORDS;
  const uint2 op = hd[3], rs = hd[4];
  if (((rs.x >> 16) & 0xFFu) != PP_ST_OK) return;
  uint8_t d[64];
  pp_digest(d, stream + res[i].off, op.x, op.y);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      lo |= (uint32_t)d[8 * k + j] << (8 * j);
      hi |= (uint32_t)d[8 * k + 4 + j] << (8 * j);
    }
    hd[13 + k] = make_uint2(lo, hi);
  }
}

hipError_t launch_pp(const uint8_t* d_stream, uint64_t stream_bytes, const void* d_res, const uint32_t* d_n_res,
                     uint32_t n_entries, void* d_pp, hipStream_t st) {
  hipLaunchKernelGGL(pp_parse_kernel, dim3(n_entries), dim3(64), 0, st, d_stream, stream_bytes,
                     (const pbft_admit_residue*)d_res, d_n_res, n_entries, (uint2*)d_pp);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pp_digest_kernel, dim3((n_entries + 63) / 64), dim3(64), 0, st, d_stream,
                     (const pbft_admit_residue*)d_res, n_entries, (uint2*)d_pp);
  return hipGetLastError();
}

// ---- the host build of the rule: one frame, no context, no GPU ----
int pbft_wire_decode_preprepare(const uint8_t* body, size_t len, pbft_pp_head* out) {
  if (!out || (!body && len)) return PBFT_EINVAL;
  memset(out, 0, sizeof *out);
  if (len < PP_FRAME_MIN || len > PP_FRAME_MAX) return PBFT_OK;
  const frame_mem_reader rd{body, 0, (uint32_t)len, 0};
  pp_fields h;
  if (wire_pp_frame(rd, pp_byte_scan<frame_mem_reader>{rd}, 0, (uint32_t)len, h) != PP_ST_OK) return PBFT_OK;
  out->view = h.view;
  out->seq = h.seq;
  out->timestamp = h.timestamp;
  out->op_off = h.op_off;
  out->op_len = h.op_len;
  out->replica = (uint16_t)h.replica;
  out->status = PBFT_PP_OK;
  memcpy(out->claimed, h.claimed, 64);
  memcpy(out->sig, h.sig, 64);
  pp_digest(out->computed, body, h.op_off, h.op_len);
  return PBFT_OK;
}
