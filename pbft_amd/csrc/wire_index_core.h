// Framing of UviBytes streams, shared by the host and the device (wire_index.hip): one connection's bytes -> body
// offset and length of every whole frame.  The accept rule of one step is that of the framing loop of
// pbft_wire_frame_index (host/wire.cpp), which stays the oracle: pbft_uvi_decode (a 10-byte overlong or > u64 varint
// and a non-minimal varint are errors, a varint cut by the end of the segment is "need more"), a length above
// PBFT_UVI_MAX_FRAME is an error, a body cut by the end of the segment is "incomplete".
//
// The walk is a chain (frame k + 1 starts where frame k ends), so it is cut into tiles of T bytes counted from the
// segment's start and put together again from per-tile tables:
//   tile table   for every entry offset e < IX_ENTRIES of a tile: where the chain that starts a frame at tile + e
//                first leaves the tile, how many frames start inside it, or where it stopped / failed;
//   group table  the same over IX group = T / 128 consecutive tiles, composed from the tile tables;
//   resolve      per segment over its groups, then per group over its tiles: every tile's real entry and the number
//                of frames in front of it;
//   emit         every tile with an entry is walked once more and its frames are written at their numbers.
// Every function here is the work of one lane; the kernels and the host build (tests/native/index_main.cpp) differ only
// in who loops over the lanes.  Bytes are read through an accessor `uint32_t B::operator()(uint64_t i) const` of
// segment-relative positions; every position is tested against the segment's length before it is read, so no byte
// outside a segment reaches a result.
#pragma once
#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__CUDACC__)
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

namespace pbft {

constexpr uint32_t IX_UVI_MAX_FRAME = 128u * 1024u * 1024u;  // PBFT_UVI_MAX_FRAME
// A canonical vote frame is at most 2 + 379 bytes: one that starts on a tile's last byte puts the next header at
// offset <= 380 of the next tile.  Entries >= IX_ENTRIES (after a PrePrepare, a ClientRequest, an adversary's frame)
// are walked from the stream's bytes by the lane that meets them.
constexpr uint32_t IX_ENTRIES = 384;
constexpr uint32_t IX_TILE_MIN = 512, IX_TILE_MAX = 16384;  // tile bytes: a power of two in this range
constexpr uint32_t IX_MAX_SEGMENTS = 65536;
constexpr uint64_t IX_MAX_STREAM = (uint64_t)1 << 31;  // frame numbers, tile numbers and counts fit 32 bits
constexpr uint32_t IX_NONE = 0xFFFFFFFFu;
enum : uint32_t { IX_GO = 0, IX_STOP = 1, IX_ERR = 2 };  // IX_STOP / IX_ERR - 1 = pbft_seg_head.status 0 / 1
constexpr uint32_t IX_SEG_OUTSIDE = 2;                   // pbft_seg_head.status: the segment is not read

__host__ __device__ inline uint32_t ix_group_tiles(uint32_t T) { return T >> 7; }  // 4 at 512, 128 at 16384

// One step at segment position at < len.  IX_GO: a whole frame, body [at + hn, at + hn + fl); IX_STOP: the varint or
// the body is cut by the segment's end; IX_ERR: framing error.
template <class B>
__host__ __device__ inline uint32_t ix_step(const B& b, uint64_t at, uint64_t len, uint32_t& hn, uint64_t& fl) {
  uint64_t v = 0;
  for (uint32_t i = 0; i < 10; ++i) {
    if (at + i >= len) return IX_STOP;  // need more bytes
    const uint32_t c = b(at + i);
    if (i == 9 && c > 1) return IX_ERR;  // > u64
    v |= (uint64_t)(c & 0x7F) << (7 * i);
    if (!(c & 0x80)) {
      if (c == 0 && i > 0) return IX_ERR;  // non-minimal
      if (v > IX_UVI_MAX_FRAME) return IX_ERR;
      hn = i + 1;
      fl = v;
      return len - at - hn < v ? IX_STOP : IX_GO;  // incomplete body: kept for the next call
    }
  }
  return IX_ERR;  // overlong
}

// What a chain does in one tile, 8 bytes.  IX_GO: val = the position it leaves the tile at, counted from the tile's
// end (the next frame's header; < 2^27 + 10 + T); else val = the position in the tile where it stopped or failed.
struct ix_hop {
  uint32_t val;
  uint32_t cs;  // frames that start in the tile (<= T) | status << 30
  __host__ __device__ uint32_t count() const { return cs & 0x3FFFFFFFu; }
  __host__ __device__ uint32_t status() const { return cs >> 30; }
};

struct ix_no_emit {
  __host__ __device__ void operator()(uint32_t, uint64_t, uint32_t) const {}
};

// The chain that starts a frame at tile_start + e (e < T), followed to the end of the tile [tile_start, tile_start +
// T).  emit(k, body, fl) for its k-th frame.  At most T hops: a hop advances by at least one byte.
template <class B, class Emit>
__host__ __device__ inline ix_hop ix_walk_tile(const B& b, uint64_t seg_len, uint64_t tile_start, uint32_t T,
                                               uint32_t e, const Emit& emit) {
  const uint64_t end = tile_start + T;
  uint64_t at = tile_start + e;
  uint32_t count = 0, status = IX_GO;
  for (uint32_t hop = 0; hop < T && at < end; ++hop) {
    if (at >= seg_len) { status = IX_STOP; break; }  // (at == seg_len: the segment ends on a frame boundary)
    uint32_t hn;
    uint64_t fl;
    status = ix_step(b, at, seg_len, hn, fl);
    if (status != IX_GO) break;
    emit(count, at + hn, (uint32_t)fl);
    ++count;
    at += hn + fl;
  }
  ix_hop r;
  r.val = (uint32_t)(status == IX_GO ? at - end : at - tile_start);
  r.cs = count | status << 30;
  return r;
}

// A chain between tiles, 16 bytes.  IX_GO: about to start a frame at byte `entry` of tile `tile` (of its segment),
// `count` frames behind it; else it stopped / failed at segment position pos = a | b << 32.
struct ix_state {
  uint32_t a, b, count, status;
  __host__ __device__ uint64_t pos() const { return (uint64_t)b << 32 | a; }
  __host__ __device__ void stop(uint32_t st, uint64_t p) { status = st; a = (uint32_t)p; b = (uint32_t)(p >> 32); }
};
__host__ __device__ inline ix_state ix_at(uint32_t tile, uint32_t entry, uint32_t count) {
  ix_state s;
  s.a = tile; s.b = entry; s.count = count; s.status = IX_GO;
  return s;
}

// One segment as the resolving lanes see it.
struct ix_seg {
  const uint8_t* bytes;  // the segment's first byte (read only at positions < len)
  uint64_t len;
  uint32_t n_tiles, T, log2T;
  const ix_hop* tab;  // the tables of the segment's tiles, IX_ENTRIES each
};
struct ix_mem_bytes {
  const uint8_t* p;
  __host__ __device__ uint32_t operator()(uint64_t i) const { return p[i]; }
};

// One tile further: by the table, or (entry >= IX_ENTRIES) by the bytes.  A chain that leaves the last tile stands at
// the segment's end: the walk is over, with status OK.
__host__ __device__ inline void ix_advance(const ix_seg& sg, ix_state& st) {
  const uint32_t tile = st.a, entry = st.b;
  const ix_hop h = entry < IX_ENTRIES ? sg.tab[(uint64_t)tile * IX_ENTRIES + entry]
                                      : ix_walk_tile(ix_mem_bytes{sg.bytes}, sg.len, (uint64_t)tile << sg.log2T, sg.T,
                                                     entry, ix_no_emit{});
  st.count += h.count();
  if (h.status() != IX_GO) {
    st.stop(h.status(), ((uint64_t)tile << sg.log2T) + h.val);
    return;
  }
  st.a = tile + 1 + (h.val >> sg.log2T);  // (a frame longer than a tile skips tiles)
  st.b = h.val & (sg.T - 1);
  if (st.a >= sg.n_tiles) st.stop(IX_STOP, ((uint64_t)st.a << sg.log2T) + st.b);  // (= len)
}

// Follow st to the first tile >= t_end (<= n_tiles) or to its stop.  At most t_end - tile hops: each advances a tile.
__host__ __device__ inline void ix_walk_range(const ix_seg& sg, ix_state& st, uint32_t t_end) {
  if (st.status != IX_GO || st.a >= t_end) return;
  const uint32_t bound = t_end - st.a;
  for (uint32_t i = 0; i < bound && st.status == IX_GO && st.a < t_end; ++i) ix_advance(sg, st);
}

// The segment (or group's segment) of global tile (group) x: the last s with base[s] <= x, for x < base[S].
// base[S + 1] is non-decreasing (an empty segment has base[s] == base[s + 1]).  At most 17 halvings (S <= 65536).
__host__ __device__ inline uint32_t ix_find_seg(const uint32_t* base, uint32_t S, uint32_t x) {
  uint32_t lo = 0, hi = S;  // the answer is in [lo, hi)
  for (uint32_t i = 0; i < 17 && hi - lo > 1; ++i) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (base[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Segment s may be read iff it lies inside the stream and the lengths of the segments up to it that lie inside add
// up to no more than the stream (run = that sum, saturating): segments that overlap cannot make more tiles than the
// workspace has.
__host__ __device__ inline bool ix_seg_inside(uint64_t off, uint64_t len, uint64_t stream_bytes) {
  return len <= stream_bytes && off <= stream_bytes - len;
}
__host__ __device__ inline uint64_t ix_sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~(uint64_t)0 : a + b; }
__host__ __device__ inline uint32_t ix_tiles_of(uint64_t len, uint32_t log2T) {
  return (uint32_t)((len + (((uint64_t)1 << log2T) - 1)) >> log2T);  // len <= IX_MAX_STREAM
}
__host__ __device__ inline uint32_t ix_groups_of(uint32_t n_tiles, uint32_t T) {
  const uint32_t G = ix_group_tiles(T);
  return (n_tiles + G - 1) / G;
}

// The per-segment record (pbft_seg_head of include/pbft_wire.h)
struct ix_head {
  uint64_t consumed;
  uint32_t first, n_frames, status, pad;
};
// Where a group / a tile is entered: entry = IX_NONE if the chain never starts a frame in it
struct ix_group_start {
  uint32_t tile, entry, count, pad;
};
struct ix_tile_start {
  uint32_t entry, count;
};

// ---- the lanes ----
// Group table: lane e of group g (tiles [t0, t1) of its segment).
__host__ __device__ inline ix_state ix_compose_lane(const ix_seg& sg, uint32_t t0, uint32_t t1, uint32_t e) {
  ix_state st = ix_at(t0, e, 0);
  ix_walk_range(sg, st, t1);
  return st;
}

// One lane per segment: over its n_groups groups, by the group tables where a group is entered at its first tile
// with entry < IX_ENTRIES, by the tile tables otherwise.  Writes every group's start and the head but for `first`.
__host__ __device__ inline void ix_resolve_segment(const ix_seg& sg, bool inside, const ix_state* gtab,
                                                   ix_group_start* gstart, ix_head* head) {
  ix_head h;
  h.consumed = 0; h.first = 0; h.n_frames = 0; h.status = IX_SEG_OUTSIDE; h.pad = 0;
  if (inside) {
    const uint32_t G = ix_group_tiles(sg.T), n_groups = ix_groups_of(sg.n_tiles, sg.T);
    ix_state st = ix_at(0, 0, 0);
    if (sg.n_tiles == 0) st.stop(IX_STOP, 0);
    for (uint32_t g = 0; g < n_groups; ++g) {
      const uint32_t t0 = g * G, t1 = t0 + G < sg.n_tiles ? t0 + G : sg.n_tiles;
      ix_group_start gs;
      gs.tile = 0; gs.entry = IX_NONE; gs.count = 0; gs.pad = 0;
      if (st.status == IX_GO && st.a < t1) {  // (st.a >= t0: the chain left the groups in front)
        gs.tile = st.a; gs.entry = st.b; gs.count = st.count;
        if (st.a == t0 && st.b < IX_ENTRIES) {
          const ix_state r = gtab[(uint64_t)g * IX_ENTRIES + st.b];
          const uint32_t c = st.count + r.count;
          st = r;
          st.count = c;
        } else {
          ix_walk_range(sg, st, t1);
        }
      }
      gstart[g] = gs;
    }
    h.consumed = st.pos();  // (every chain of a segment ends in a stop: ix_advance)
    h.n_frames = st.count;
    h.status = st.status - 1;
  }
  *head = h;
}

// One lane per group: every tile's entry and the frames of the segment in front of it.
__host__ __device__ inline void ix_resolve_group(const ix_seg& sg, uint32_t t0, uint32_t t1, const ix_group_start& gs,
                                                 ix_tile_start* tstart) {
  ix_state st = ix_at(gs.tile, gs.entry, gs.count);
  if (gs.entry == IX_NONE) st.stop(IX_STOP, 0);
  for (uint32_t t = t0; t < t1; ++t) {
    ix_tile_start ts;
    ts.entry = IX_NONE; ts.count = 0;
    if (st.status == IX_GO && st.a == t) {
      ts.entry = st.b; ts.count = st.count;
      ix_advance(sg, st);
    }
    tstart[t] = ts;
  }
}

// One lane per entered tile: its frames, numbered first + k, written while the number is below frame_cap.
struct ix_emit_out {
  uint64_t* off;
  uint32_t* len;
  uint16_t* peer;
  uint64_t seg_off, frame_cap;
  uint32_t first, peer_of_seg;
  __host__ __device__ void operator()(uint32_t k, uint64_t body, uint32_t fl) const {
    const uint64_t f = (uint64_t)first + k;
    if (f >= frame_cap) return;
    off[f] = seg_off + body;
    len[f] = fl;
    if (peer) peer[f] = (uint16_t)peer_of_seg;
  }
};

}  // namespace pbft
