// Frame decoder (include/pbft_wire.h pbft_wire_decode_frames_device): the canonical signed-vote JSON frame of the
// reference's wire (UviBytes + serde_json, src/protocol_config.rs:49-69, :125-129) parsed on the GPU into the binary
// records pbft_verify_records_device consumes, so that a vote's bytes are never touched by the host.
// Its own translation unit; plain C++ (16-byte loads, LDS, 16- and 8-byte stores).
#include "wire_decode_kernels.h"

#include "../../include/pbft_wire.h"
#include "wire_decode_core.h"

using namespace pbft;

static_assert(WIRE_ST_OK == PBFT_WIRE_OK && WIRE_ST_ESIGNER == PBFT_WIRE_ESIGNER && WIRE_ST_EDEFER == PBFT_WIRE_EDEFER,
              "the core's status values are the header's");
static_assert(FRAME_MIN == PBFT_FRAME_MIN && FRAME_MAX == PBFT_FRAME_MAX, "the core's length window is the header's");
static_assert(sizeof(pbft_frame_head) == 24 && PBFT_RECORD_BYTES == 160, "three 8-byte, ten 16-byte stores per frame");

static constexpr uint32_t ROW = FRAME_ROW_DWORDS;
// a frame of at most 379 bytes that starts anywhere in a 16-byte granule spans at most ceil((15 + 379) / 16) of them
static constexpr uint32_t GRANULES = 25;

struct lds_row {
  const uint32_t* row;
  __device__ __forceinline__ uint32_t dword(uint32_t i) const { return row[i]; }
};

// One lane per frame, one wave per block.
//  1. Each lane checks its frame's bounds: 336 <= len <= 379 and off + len <= stream_bytes, before any address is
//     formed.  A frame that fails is PBFT_WIRE_EDEFER and none of its bytes are read.
//  2. The wave stages its 64 frames into LDS: task t = 25 fr + g is granule g of frame fr, so consecutive lanes load
//     consecutive 16-byte granules (frames packed back to back: one contiguous span; with gaps or out of order the
//     same code, each frame located by its own offset).  Only granules that hold a byte of a frame are loaded (and
//     the stream's first one), all inside [d_stream, d_stream + round_up(stream_bytes, 16)).  A granule's four dwords
//     go to the frame's row shifted by whole dwords, so that the frame starts at byte off % 4 of the row: rows of 97
//     dwords (wire_decode_core.h).
//  3. Each lane parses its own row (aligned LDS dwords and a byte shift) and writes its record as ten 16-byte stores
//     and its head as three 8-byte stores.
__global__ void __launch_bounds__(FRAMES_BLOCK) decode_frames_kernel(const uint8_t* __restrict__ stream,
                                                                     uint64_t stream_bytes,
                                                                     const uint64_t* __restrict__ off,
                                                                     const uint32_t* __restrict__ len,
                                                                     const uint16_t* __restrict__ peer,
                                                                     uint32_t n_replicas, uint64_t N,
                                                                     uint4* __restrict__ records,
                                                                     uint2* __restrict__ heads) {
  __shared__ uint32_t rows[FRAMES_BLOCK * ROW];
  __shared__ uint64_t s_off[FRAMES_BLOCK];
  __shared__ uint32_t s_len[FRAMES_BLOCK];
  const uint32_t lane = threadIdx.x;
  const uint64_t f = (uint64_t)blockIdx.x * FRAMES_BLOCK + lane;
  uint64_t o = 0;
  uint32_t flen = 0, L = 0;  // L: the length if the frame may be read, else 0
  if (f < N) {
    flen = len[f];
    if (flen >= FRAME_MIN && flen <= FRAME_MAX && stream_bytes >= flen) {
      o = off[f];
      if (o <= stream_bytes - flen) L = flen;
    }
  }
  s_off[lane] = o;
  s_len[lane] = L;
  __syncthreads();
  // All 25 loads of a lane are issued before the first is used: at 25.6 KB of LDS per wave a CU holds six waves, too
  // few to hide one memory round trip per granule behind each other (measured: profiles/frames/README.md).
  if (stream_bytes) {  // (wave-uniform)
    uint4 v[GRANULES];
    uint32_t slot[GRANULES];  // LDS dword index of the granule's first dword; NONE: no byte of a readable frame in it
    constexpr uint32_t NONE = 0x80000000u;
#pragma unroll
    for (uint32_t r = 0; r < GRANULES; ++r) {
      const uint32_t t = r * FRAMES_BLOCK + lane;
      const uint32_t fr = t / GRANULES, g = t - fr * GRANULES;
      const uint32_t Lf = s_len[fr];
      const uint64_t of = s_off[fr];
      const uint32_t a = (uint32_t)of & 15u;
      const bool on = Lf != 0 && 16 * g < a + Lf;
      // (+ 4: up to 3 dwords of a frame's first granule lie in front of its row; the offset keeps their index from
      // wrapping, and the range test below drops them)
      slot[r] = on ? fr * ROW + 4 * g - (a >> 2) + 4 : NONE;
      // (unconditional, so that nothing waits for it here: a task without a granule reads the stream's first one,
      // which a stream that is not empty has)
      v[r] = *(const uint4*)(stream + (on ? (of - a) + 16 * g : 0));
    }
#pragma unroll
    for (uint32_t r = 0; r < GRANULES; ++r) {
      // (all four dwords count as used: hipcc otherwise splits the load by which of the stores below may run)
      asm volatile("" : "+v"(v[r].x), "+v"(v[r].y), "+v"(v[r].z), "+v"(v[r].w));
      if (slot[r] == NONE) continue;
      const uint32_t t = r * FRAMES_BLOCK + lane;
      const uint32_t lo = (t / GRANULES) * ROW + 4, hi = lo + ROW;  // the row's dwords, in slot's + 4 numbering
      const uint32_t d = slot[r];
      if (d >= lo && d < hi) rows[d - 4] = v[r].x;
      if (d + 1 >= lo && d + 1 < hi) rows[d - 3] = v[r].y;
      if (d + 2 >= lo && d + 2 < hi) rows[d - 2] = v[r].z;
      if (d + 3 >= lo && d + 3 < hi) rows[d - 1] = v[r].w;
    }
  }
  __syncthreads();
  if (f >= N) return;
  uint32_t pr = FRAME_NO_PEER;
  if (peer) pr = peer[f];
  uint32_t rec[40];
  frame_fields h;
  wire_decode_frame(lds_row{rows + lane * ROW}, (uint32_t)o & 3u, L, n_replicas, pr, rec, h);
  // (each lane stores its own record: sending the records through LDS to store them as contiguous runs of the wave
  // measured the same, profiles/frames/README.md)
  uint4* dst = records + f * 10;
#pragma unroll
  for (int k = 0; k < 10; ++k) dst[k] = make_uint4(rec[4 * k], rec[4 * k + 1], rec[4 * k + 2], rec[4 * k + 3]);
  uint2* hd = heads + f * 3;
  hd[0] = make_uint2((uint32_t)h.view, (uint32_t)(h.view >> 32));
  hd[1] = make_uint2((uint32_t)h.seq, (uint32_t)(h.seq >> 32));
  hd[2] = make_uint2(h.key_idx | (h.kind << 16) | (h.status << 24), flen);
}

// 13 lanes per patch: ten 16-byte granules of the record, three 8-byte words of the head
__global__ void __launch_bounds__(256) patch_frames_kernel(const uint32_t* __restrict__ idx,
                                                           const uint4* __restrict__ prec,
                                                           const uint2* __restrict__ phead, uint32_t P, uint64_t N,
                                                           uint4* __restrict__ records, uint2* __restrict__ heads) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t p = t / 13;
  const uint32_t k = (uint32_t)(t - p * 13);
  if (p >= P) return;
  const uint64_t f = idx[p];
  if (f >= N) return;
  if (k < 10) records[f * 10 + k] = prec[p * 10 + k];
  else heads[f * 3 + (k - 10)] = phead[p * 3 + (k - 10)];
}

hipError_t launch_decode_frames(const uint8_t* d_stream, uint64_t stream_bytes, const uint64_t* d_off,
                                const uint32_t* d_len, const uint16_t* d_peer, uint32_t n_replicas, uint64_t N,
                                uint8_t* d_records, void* d_heads, hipStream_t st) {
  hipLaunchKernelGGL(decode_frames_kernel, dim3((unsigned)((N + FRAMES_BLOCK - 1) / FRAMES_BLOCK)), dim3(FRAMES_BLOCK),
                     0, st, d_stream, stream_bytes, d_off, d_len, d_peer, n_replicas, N, (uint4*)d_records,
                     (uint2*)d_heads);
  return hipGetLastError();
}

hipError_t launch_patch_frames(const uint32_t* d_idx, const uint8_t* d_prec, const void* d_phead, uint32_t P,
                               uint64_t N, uint8_t* d_records, void* d_heads, hipStream_t st) {
  const uint64_t threads = (uint64_t)P * 13;
  hipLaunchKernelGGL(patch_frames_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, d_idx,
                     (const uint4*)d_prec, (const uint2*)d_phead, P, N, (uint4*)d_records, (uint2*)d_heads);
  return hipGetLastError();
}
