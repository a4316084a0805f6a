// Launcher of the stream index (wire_index.hip): S segments of a byte stream -> body offset, length and peer of every
// whole UviBytes frame, one head per segment, the totals.  Called by pbft_wire_index_streams_device
// (pbft_verify.hip), which owns the workspace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wire_index_core.h"

static constexpr uint32_t INDEX_TILE_DEFAULT = pbft::IX_TILE_MAX;
static constexpr int INDEX_SCAN_BLOCK = 1024;  // the one block that prefix-sums over the segments, 64 per lane

// The workspace of one call, carved from a context buffer: tile base, group base and "inside" flag per segment | the
// tile tables | the group tables | every group's and every tile's start.  Monotone in stream_bytes and in S for a
// fixed tile size: a buffer reserved for (max_stream_bytes, max_segments) holds every smaller call.
struct index_ws {
  uint32_t T, log2T;
  uint64_t tile_cap, group_cap;  // segments that lie inside the stream have no more tiles / groups than this
  size_t off_group_base, off_inside, off_tab, off_gtab, off_gstart, off_tstart, total;
  index_ws(uint64_t stream_bytes, uint32_t S, uint32_t tile) {
    T = tile;
    log2T = 0;
    while (((uint32_t)1 << log2T) < T) ++log2T;
    tile_cap = ((stream_bytes + T - 1) >> log2T) + S;
    const uint32_t G = pbft::ix_group_tiles(T);
    group_cap = (tile_cap + G - 1) / G + S;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    off_group_base = up(4 * ((size_t)S + 1));
    off_inside = off_group_base + up(4 * ((size_t)S + 1));
    off_tab = off_inside + up(4 * (size_t)S);
    off_gtab = off_tab + up(sizeof(pbft::ix_hop) * pbft::IX_ENTRIES * (size_t)tile_cap);
    off_gstart = off_gtab + up(sizeof(pbft::ix_state) * pbft::IX_ENTRIES * (size_t)group_cap);
    off_tstart = off_gstart + up(sizeof(pbft::ix_group_start) * (size_t)group_cap);
    total = off_tstart + up(sizeof(pbft::ix_tile_start) * (size_t)tile_cap);
  }
};

// Up to eight kernel launches on st (setup, tile tables, group tables, segments, totals, groups, emit, pad); no
// allocation, copy, memset or synchronisation.  ws holds index_ws(stream_bytes, S, tile).total bytes, 256-byte
// aligned.  stream_bytes <= 2^31, S <= 65536, frame_cap <= 2^31; heads = pbft_seg_head[S]; n_frames = uint32_t[2].
hipError_t launch_index_streams(const uint8_t* d_stream, uint64_t stream_bytes, const uint64_t* d_seg_off,
                                const uint64_t* d_seg_len, const uint16_t* d_seg_peer, uint32_t S, uint64_t frame_cap,
                                uint32_t tile, uint8_t* ws, uint64_t* d_off, uint32_t* d_len, uint16_t* d_peer,
                                void* d_heads, uint32_t* d_n_frames, hipStream_t st);
