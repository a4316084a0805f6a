// Stream index (include/pbft_wire.h pbft_wire_index_streams_device): the varint walk of pbft_wire_frame_index on the
// GPU, over S connection segments of one byte stream at once.  The scheme and every lane's work are in
// wire_index_core.h; here are the kernels that loop over the lanes, the staging of a tile into LDS and the two
// prefix sums over the segments.  Its own translation unit; plain C++ (16-byte loads, LDS, 16-, 8-, 4- and 2-byte
// stores).  The phases meet only at kernel boundaries: no lane waits for a value another block writes, and every
// word of the workspace that a kernel reads was written by a kernel in front of it in the same call.
#include "wire_index_kernels.h"

#include "../../include/pbft_wire.h"

using namespace pbft;

static_assert(IX_UVI_MAX_FRAME == PBFT_UVI_MAX_FRAME, "the core's frame limit is the header's");
static_assert(sizeof(pbft_seg_head) == 24 && sizeof(ix_head) == 24, "one 24-byte head per segment");
static_assert(sizeof(ix_hop) == 8 && sizeof(ix_state) == 16 && sizeof(ix_group_start) == 16 &&
                  sizeof(ix_tile_start) == 8,
              "table entries are one 8- or 16-byte access");
static_assert(IX_MAX_SEGMENTS == 64 * INDEX_SCAN_BLOCK, "the scan block covers every segment, 64 per lane");

struct index_args {
  const uint8_t* stream;
  uint64_t stream_bytes;
  const uint64_t* seg_off;
  const uint64_t* seg_len;
  const uint16_t* seg_peer;
  uint32_t S, T, log2T;
  uint64_t frame_cap;
  uint32_t* tile_base;   // [S + 1]
  uint32_t* group_base;  // [S + 1]
  uint32_t* inside;      // [S]
  ix_hop* tab;           // [tiles][IX_ENTRIES]
  ix_state* gtab;        // [groups][IX_ENTRIES]
  ix_group_start* gstart;
  ix_tile_start* tstart;
  uint64_t* off;
  uint32_t* len;
  uint16_t* peer;
  ix_head* heads;
  uint32_t* n_frames;
};

// Exclusive prefix of one value per lane over the block (INDEX_SCAN_BLOCK lanes); *total = the sum.  Saturating.
__device__ static uint64_t block_scan(uint64_t v, uint64_t* sh, uint64_t* total) {
  const uint32_t t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < INDEX_SCAN_BLOCK; d <<= 1) {
    const uint64_t x = t >= d ? sh[t - d] : 0;
    __syncthreads();
    sh[t] = ix_sat_add(sh[t], x);
    __syncthreads();
  }
  const uint64_t ex = t ? sh[t - 1] : 0;
  *total = sh[INDEX_SCAN_BLOCK - 1];
  __syncthreads();
  return ex;
}

// One block.  Lane t owns segments [64 t, 64 t + 64): which of them may be read (ix_seg_inside and the running sum
// of lengths), their tile and group counts, and the exclusive prefixes of both.
__global__ void __launch_bounds__(INDEX_SCAN_BLOCK) index_setup_kernel(index_args a) {
  __shared__ uint64_t sh[INDEX_SCAN_BLOCK];
  const uint32_t lo = threadIdx.x * 64, hi = lo + 64 < a.S ? lo + 64 : a.S;
  uint64_t sum = 0, total;
  for (uint32_t s = lo; s < hi; ++s) {
    const uint64_t l = a.seg_len[s];
    if (ix_seg_inside(a.seg_off[s], l, a.stream_bytes)) sum = ix_sat_add(sum, l);
  }
  uint64_t run = block_scan(sum, sh, &total);
  uint64_t counts = 0;  // tiles << 32 | groups
  for (uint32_t s = lo; s < hi; ++s) {
    const uint64_t l = a.seg_len[s];
    bool in = ix_seg_inside(a.seg_off[s], l, a.stream_bytes);
    if (in) {
      run = ix_sat_add(run, l);
      in = run <= a.stream_bytes;
    }
    a.inside[s] = in;
    if (in) {
      const uint32_t nt = ix_tiles_of(l, a.log2T);
      counts += (uint64_t)nt << 32 | ix_groups_of(nt, a.T);
    }
  }
  uint64_t base = block_scan(counts, sh, &total);
  for (uint32_t s = lo; s < hi; ++s) {
    a.tile_base[s] = (uint32_t)(base >> 32);
    a.group_base[s] = (uint32_t)base;
    if (a.inside[s]) {  // (this lane's own store)
      const uint32_t nt = ix_tiles_of(a.seg_len[s], a.log2T);
      base += (uint64_t)nt << 32 | ix_groups_of(nt, a.T);
    }
  }
  if (threadIdx.x == 0) {
    a.tile_base[a.S] = (uint32_t)(total >> 32);
    a.group_base[a.S] = (uint32_t)total;
  }
}

__device__ static ix_seg seg_of(const index_args& a, uint32_t s) {
  ix_seg sg;
  sg.bytes = a.stream + a.seg_off[s];
  sg.len = a.seg_len[s];
  sg.n_tiles = a.tile_base[s + 1] - a.tile_base[s];
  sg.T = a.T;
  sg.log2T = a.log2T;
  sg.tab = a.tab + (uint64_t)a.tile_base[s] * IX_ENTRIES;
  return sg;
}

// A tile in LDS: the 16-byte granules of the stream that hold bytes [tile_start, tile_start + T + 9) of the segment
// (the 9: a varint that starts on the tile's last byte), cut at the segment's end.  All of them lie inside
// [stream, stream + round_up(stream_bytes, 16)), because the segment lies inside stream_bytes.
static constexpr uint32_t TILE_GRANULES = IX_TILE_MAX / 16 + 3;  // ceil((15 + T + 9) / 16) = T / 16 + 2
struct lds_bytes {
  const uint8_t* lds;
  uint64_t origin;  // the segment position that lds[0] holds (mod 2^64: the first granule may begin in front of it)
  __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return lds[(uint32_t)(i - origin)]; }
};
__device__ static lds_bytes stage_tile(uint4* lds, const index_args& a, uint32_t s, const ix_seg& sg,
                                       uint64_t tile_start) {
  const uint64_t g0 = a.seg_off[s] + tile_start;  // the tile's first byte in the stream (tile_start < len)
  const uint64_t rest = sg.len - tile_start;
  const uint64_t need = rest < (uint64_t)sg.T + 9 ? rest : (uint64_t)sg.T + 9;
  const uint64_t a0 = g0 & ~(uint64_t)15, a1 = (g0 + need + 15) & ~(uint64_t)15;
  uint32_t n = (uint32_t)((a1 - a0) >> 4);
  if (n > TILE_GRANULES) n = TILE_GRANULES;  // (never: see TILE_GRANULES)
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) lds[i] = *(const uint4*)(a.stream + a0 + 16 * (uint64_t)i);
  __syncthreads();
  // segment position p is stream byte seg_off + p = a0 + (p - tile_start) + (g0 - a0)
  return lds_bytes{(const uint8_t*)lds, tile_start - (g0 - a0)};
}

// Phase 1, one block per tile, one lane per entry offset: the tile's table.
__global__ void __launch_bounds__(IX_ENTRIES) index_tables_kernel(index_args a) {
  __shared__ uint4 lds[TILE_GRANULES];
  const uint32_t x = blockIdx.x;
  if (x >= a.tile_base[a.S]) return;  // (block-uniform)
  const uint32_t s = ix_find_seg(a.tile_base, a.S, x);
  const ix_seg sg = seg_of(a, s);
  const uint64_t tile_start = (uint64_t)(x - a.tile_base[s]) << a.log2T;
  const lds_bytes b = stage_tile(lds, a, s, sg, tile_start);
  const uint32_t e = threadIdx.x;
  a.tab[(uint64_t)x * IX_ENTRIES + e] = ix_walk_tile(b, sg.len, tile_start, sg.T, e, ix_no_emit{});
}

// Phase 2a, one block per group, one lane per entry offset: the group's table, composed from its tiles' tables.
__global__ void __launch_bounds__(IX_ENTRIES) index_compose_kernel(index_args a) {
  const uint32_t x = blockIdx.x;
  if (x >= a.group_base[a.S]) return;
  const uint32_t s = ix_find_seg(a.group_base, a.S, x);
  const ix_seg sg = seg_of(a, s);
  const uint32_t G = ix_group_tiles(a.T), t0 = (x - a.group_base[s]) * G;
  const uint32_t t1 = t0 + G < sg.n_tiles ? t0 + G : sg.n_tiles;
  const ix_state r = ix_compose_lane(sg, t0, t1, threadIdx.x);
  *(uint4*)&a.gtab[(uint64_t)x * IX_ENTRIES + threadIdx.x] = make_uint4(r.a, r.b, r.count, r.status);
}

// Phase 2b, one lane per segment: its groups' starts, its frame count, consumed bytes and status.
__global__ void __launch_bounds__(64) index_segments_kernel(index_args a) {
  const uint32_t s = blockIdx.x * 64 + threadIdx.x;
  if (s >= a.S) return;
  const ix_seg sg = seg_of(a, s);
  const uint32_t gb = a.group_base[s];
  ix_resolve_segment(sg, a.inside[s] != 0, a.gtab + (uint64_t)gb * IX_ENTRIES, a.gstart + gb, a.heads + s);
}

// Phase 2c, one block: `first` of every head = the exclusive prefix of the frame counts; the totals.
__global__ void __launch_bounds__(INDEX_SCAN_BLOCK) index_totals_kernel(index_args a) {
  __shared__ uint64_t sh[INDEX_SCAN_BLOCK];
  const uint32_t lo = threadIdx.x * 64, hi = lo + 64 < a.S ? lo + 64 : a.S;
  uint64_t sum = 0, total;
  for (uint32_t s = lo; s < hi; ++s) sum += a.heads[s].n_frames;
  uint64_t first = block_scan(sum, sh, &total);  // (<= IX_MAX_STREAM: the segments read add up to no more bytes)
  for (uint32_t s = lo; s < hi; ++s) {
    a.heads[s].first = (uint32_t)first;
    first += a.heads[s].n_frames;
  }
  if (threadIdx.x == 0) {
    a.n_frames[0] = (uint32_t)total;
    a.n_frames[1] = total > a.frame_cap ? (uint32_t)(total - a.frame_cap) : 0;
  }
}

// Phase 2d, one lane per group: its tiles' starts.
__global__ void __launch_bounds__(64) index_groups_kernel(index_args a) {
  const uint32_t x = blockIdx.x * 64 + threadIdx.x;
  if (x >= a.group_base[a.S]) return;
  const uint32_t s = ix_find_seg(a.group_base, a.S, x);
  const ix_seg sg = seg_of(a, s);
  const uint32_t G = ix_group_tiles(a.T), t0 = (x - a.group_base[s]) * G;
  const uint32_t t1 = t0 + G < sg.n_tiles ? t0 + G : sg.n_tiles;
  ix_resolve_group(sg, t0, t1, a.gstart[x], a.tstart + a.tile_base[s]);
}

// Phase 3, one block per tile: staged as in phase 1, then one lane walks it from its entry and writes its frames.
static constexpr int INDEX_EMIT_BLOCK = 256;
__global__ void __launch_bounds__(INDEX_EMIT_BLOCK) index_emit_kernel(index_args a) {
  __shared__ uint4 lds[TILE_GRANULES];
  const uint32_t x = blockIdx.x;
  if (x >= a.tile_base[a.S]) return;
  const ix_tile_start ts = a.tstart[x];
  if (ts.entry == IX_NONE) return;  // (block-uniform)
  const uint32_t s = ix_find_seg(a.tile_base, a.S, x);
  const ix_seg sg = seg_of(a, s);
  const uint64_t tile_start = (uint64_t)(x - a.tile_base[s]) << a.log2T;
  const lds_bytes b = stage_tile(lds, a, s, sg, tile_start);
  if (threadIdx.x != 0) return;
  ix_emit_out out;
  out.off = a.off; out.len = a.len; out.peer = a.peer;
  out.seg_off = a.seg_off[s];
  out.frame_cap = a.frame_cap;
  out.first = a.heads[s].first + ts.count;
  out.peer_of_seg = a.seg_peer ? a.seg_peer[s] : 0;
  ix_walk_tile(b, sg.len, tile_start, sg.T, ts.entry, out);
}

// The entries behind the last frame: off 0, len 0, peer 0xFFFF (the decoder defers such a frame without reading it)
__global__ void __launch_bounds__(256) index_pad_kernel(index_args a) {
  const uint64_t f = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= a.frame_cap || f < a.n_frames[0]) return;
  a.off[f] = 0;
  a.len[f] = 0;
  if (a.peer) a.peer[f] = 0xFFFF;
}

hipError_t launch_index_streams(const uint8_t* d_stream, uint64_t stream_bytes, const uint64_t* d_seg_off,
                                const uint64_t* d_seg_len, const uint16_t* d_seg_peer, uint32_t S, uint64_t frame_cap,
                                uint32_t tile, uint8_t* ws, uint64_t* d_off, uint32_t* d_len, uint16_t* d_peer,
                                void* d_heads, uint32_t* d_n_frames, hipStream_t st) {
  const index_ws w(stream_bytes, S, tile);
  index_args a;
  a.stream = d_stream; a.stream_bytes = stream_bytes;
  a.seg_off = d_seg_off; a.seg_len = d_seg_len; a.seg_peer = d_seg_peer;
  a.S = S; a.T = w.T; a.log2T = w.log2T;
  a.frame_cap = frame_cap;
  a.tile_base = (uint32_t*)ws;
  a.group_base = (uint32_t*)(ws + w.off_group_base);
  a.inside = (uint32_t*)(ws + w.off_inside);
  a.tab = (ix_hop*)(ws + w.off_tab);
  a.gtab = (ix_state*)(ws + w.off_gtab);
  a.gstart = (ix_group_start*)(ws + w.off_gstart);
  a.tstart = (ix_tile_start*)(ws + w.off_tstart);
  a.off = d_off; a.len = d_len; a.peer = d_peer;
  a.heads = (ix_head*)d_heads;
  a.n_frames = d_n_frames;
  const unsigned tiles = (unsigned)w.tile_cap, groups = (unsigned)w.group_cap;
  if (S) {
    hipLaunchKernelGGL(index_setup_kernel, dim3(1), dim3(INDEX_SCAN_BLOCK), 0, st, a);
    if (tiles) hipLaunchKernelGGL(index_tables_kernel, dim3(tiles), dim3(IX_ENTRIES), 0, st, a);
    if (groups) hipLaunchKernelGGL(index_compose_kernel, dim3(groups), dim3(IX_ENTRIES), 0, st, a);
    hipLaunchKernelGGL(index_segments_kernel, dim3((S + 63) / 64), dim3(64), 0, st, a);
  }
  hipLaunchKernelGGL(index_totals_kernel, dim3(1), dim3(INDEX_SCAN_BLOCK), 0, st, a);
  if (S && frame_cap) {
    if (groups) hipLaunchKernelGGL(index_groups_kernel, dim3((groups + 63) / 64), dim3(64), 0, st, a);
    if (tiles) hipLaunchKernelGGL(index_emit_kernel, dim3(tiles), dim3(INDEX_EMIT_BLOCK), 0, st, a);
  }
  if (frame_cap)
    hipLaunchKernelGGL(index_pad_kernel, dim3((unsigned)((frame_cap + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}
