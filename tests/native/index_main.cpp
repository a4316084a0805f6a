// TEST INFRASTRUCTURE: the host build of the stream index (pbft_amd/csrc/wire_index_core.h, the code each GPU lane runs
// in wire_index.hip: the step, the tile tables, the composition, the resolve and the emit) under AddressSanitizer +
// UndefinedBehaviorSanitizer, against the host's own framing loop pbft_wire_frame_index (wire.cpp).  Built and run
// by tests/test_index.py, host only.  Here the loops over blocks and lanes are plain loops; every segment lies in a
// heap buffer of exactly its length, so any read outside it is a heap overflow.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../include/pbft_replica.h"
#include "../../include/pbft_wire.h"
#include "../../pbft_amd/csrc/wire_index_core.h"

using namespace pbft;

#define CHECK(c)                                                             \
  do {                                                                       \
    if (!(c)) {                                                              \
      fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); \
      exit(1);                                                               \
    }                                                                        \
  } while (0)

// wire.cpp's pbft_wire_decode_votes needs it; not used here
extern "C" void pbft_envelope(uint8_t out[PBFT_ENVELOPE_BYTES], uint8_t kind, uint64_t view, uint64_t seq,
                              const uint8_t digest[64]) {
  memcpy(out, "PBFT", 4);
  out[4] = kind;
  for (int i = 0; i < 8; ++i) out[5 + i] = (uint8_t)(view >> (8 * i));
  for (int i = 0; i < 8; ++i) out[13 + i] = (uint8_t)(seq >> (8 * i));
  memcpy(out + 21, digest, 64);
}

static std::mt19937_64 rng(20261019);
static uint64_t below(uint64_t n) { return rng() % n; }

typedef std::vector<uint8_t> Bytes;

struct Segment {
  std::unique_ptr<uint8_t[]> buf;  // exactly len bytes
  uint64_t len = 0, off = 0;       // off: where the segment claims to lie in the stream
  uint16_t peer = 0;
  bool inside = true;
};

struct Index {
  std::vector<uint64_t> off;
  std::vector<uint32_t> len;
  std::vector<uint16_t> peer;
  std::vector<ix_head> heads;
  uint32_t n_frames[2];
};

// What launch_index_streams enqueues, lane by lane.
static Index host_index(const std::vector<Segment>& segs, uint64_t stream_bytes, uint32_t T, uint64_t frame_cap) {
  const uint32_t S = (uint32_t)segs.size();
  uint32_t log2T = 0;
  while ((1u << log2T) < T) ++log2T;
  const uint32_t G = ix_group_tiles(T);
  // setup
  std::vector<uint32_t> tile_base(S + 1), group_base(S + 1), inside(S);
  uint64_t run = 0;
  uint32_t tiles = 0, groups = 0;
  for (uint32_t s = 0; s < S; ++s) {
    bool in = segs[s].inside && ix_seg_inside(segs[s].off, segs[s].len, stream_bytes);
    if (in) {
      run = ix_sat_add(run, segs[s].len);
      in = run <= stream_bytes;
    }
    inside[s] = in;
    tile_base[s] = tiles;
    group_base[s] = groups;
    if (in) {
      const uint32_t nt = ix_tiles_of(segs[s].len, log2T);
      tiles += nt;
      groups += ix_groups_of(nt, T);
    }
  }
  tile_base[S] = tiles;
  group_base[S] = groups;
  CHECK(tiles <= ((stream_bytes + T - 1) >> log2T) + S);
  CHECK(groups <= (((stream_bytes + T - 1) >> log2T) + S + G - 1) / G + S);
  std::vector<ix_hop> tab((size_t)tiles * IX_ENTRIES);
  std::vector<ix_state> gtab((size_t)groups * IX_ENTRIES);
  std::vector<ix_group_start> gstart(groups);
  std::vector<ix_tile_start> tstart(tiles);
  auto seg_of = [&](uint32_t s) {
    ix_seg sg;
    sg.bytes = segs[s].buf.get();
    sg.len = segs[s].len;
    sg.n_tiles = tile_base[s + 1] - tile_base[s];
    sg.T = T;
    sg.log2T = log2T;
    sg.tab = tab.data() + (size_t)tile_base[s] * IX_ENTRIES;
    return sg;
  };
  // phase 1
  for (uint32_t x = 0; x < tiles; ++x) {
    const uint32_t s = ix_find_seg(tile_base.data(), S, x);
    CHECK(tile_base[s] <= x && x < tile_base[s + 1]);
    const ix_seg sg = seg_of(s);
    const uint64_t tile_start = (uint64_t)(x - tile_base[s]) << log2T;
    for (uint32_t e = 0; e < IX_ENTRIES; ++e)
      tab[(size_t)x * IX_ENTRIES + e] = ix_walk_tile(ix_mem_bytes{sg.bytes}, sg.len, tile_start, T, e, ix_no_emit{});
  }
  // phase 2a
  for (uint32_t x = 0; x < groups; ++x) {
    const uint32_t s = ix_find_seg(group_base.data(), S, x);
    CHECK(group_base[s] <= x && x < group_base[s + 1]);
    const ix_seg sg = seg_of(s);
    const uint32_t t0 = (x - group_base[s]) * G, t1 = t0 + G < sg.n_tiles ? t0 + G : sg.n_tiles;
    for (uint32_t e = 0; e < IX_ENTRIES; ++e) gtab[(size_t)x * IX_ENTRIES + e] = ix_compose_lane(sg, t0, t1, e);
  }
  Index r;
  r.heads.resize(S);
  // phase 2b
  for (uint32_t s = 0; s < S; ++s)
    ix_resolve_segment(seg_of(s), inside[s] != 0, gtab.data() + (size_t)group_base[s] * IX_ENTRIES,
                       gstart.data() + group_base[s], &r.heads[s]);
  // phase 2c
  uint64_t total = 0;
  for (uint32_t s = 0; s < S; ++s) {
    r.heads[s].first = (uint32_t)total;
    total += r.heads[s].n_frames;
  }
  r.n_frames[0] = (uint32_t)total;
  r.n_frames[1] = total > frame_cap ? (uint32_t)(total - frame_cap) : 0;
  // phase 2d
  for (uint32_t x = 0; x < groups; ++x) {
    const uint32_t s = ix_find_seg(group_base.data(), S, x);
    const ix_seg sg = seg_of(s);
    const uint32_t t0 = (x - group_base[s]) * G, t1 = t0 + G < sg.n_tiles ? t0 + G : sg.n_tiles;
    ix_resolve_group(sg, t0, t1, gstart[x], tstart.data() + tile_base[s]);
  }
  // phase 3: outputs of exactly frame_cap entries, poisoned
  r.off.assign(frame_cap, 0xDEADDEADDEADDEADull);
  r.len.assign(frame_cap, 0xDEADDEADu);
  r.peer.assign(frame_cap, 0xDEAD);
  for (uint32_t x = 0; x < tiles; ++x) {
    if (tstart[x].entry == IX_NONE) continue;
    const uint32_t s = ix_find_seg(tile_base.data(), S, x);
    const ix_seg sg = seg_of(s);
    ix_emit_out out;
    out.off = r.off.data(); out.len = r.len.data(); out.peer = r.peer.data();
    out.seg_off = segs[s].off;
    out.frame_cap = frame_cap;
    out.first = r.heads[s].first + tstart[x].count;
    out.peer_of_seg = segs[s].peer;
    ix_walk_tile(ix_mem_bytes{sg.bytes}, sg.len, (uint64_t)(x - tile_base[s]) << log2T, T, tstart[x].entry, out);
  }
  for (uint64_t f = total; f < frame_cap; ++f) {
    r.off[f] = 0;
    r.len[f] = 0;
    r.peer[f] = 0xFFFF;
  }
  return r;
}

// ---- streams ----
static void put_varint(Bytes& b, uint64_t v) {
  uint8_t h[10];
  const size_t n = pbft_uvi_encode(v, h);
  b.insert(b.end(), h, h + n);
}
static void put_frame(Bytes& b, uint64_t len) {
  put_varint(b, len);
  // bodies full of bytes that look like headers: small values, continuation bytes, zeroes, '{'
  static const uint8_t FILL[] = {0x00, 0x01, 0x7B, 0x80, 0xFF, 0x81, 0x02, 0xD4};
  const uint64_t mode = below(3);
  for (uint64_t i = 0; i < len; ++i) b.push_back(mode == 0 ? (uint8_t)rng() : mode == 1 ? FILL[below(8)] : 0x80);
}
static uint64_t pick_len(bool allow_long) {
  switch (below(allow_long ? 12 : 10)) {
    case 0: return 0;
    case 1: return 1;
    case 2: return 127;
    case 3: return 128;
    case 10: return below(2) ? 16383 : 16384;
    case 11: return below(4) ? 1000 + below(200) : 69990 + below(20);
    default: return 336 + below(44);
  }
}

static const int N_TAILS = 18;
static size_t n_tail_seen[N_TAILS], n_err, n_stop_mid, n_tile_edge_err;
// tail class -> bytes appended behind whole frames; err: the host must return PBFT_EINVAL there
static void put_tail(Bytes& b, int cls) {
  if (cls >= 1 && cls <= 11) {  // 0x80 x k: need more (k <= 9), > u64 / overlong (k = 10, 11)
    b.insert(b.end(), (size_t)cls, 0x80);
  } else if (cls == 12) {  // non-minimal
    b.push_back(0x80);
    b.push_back(0x00);
  } else if (cls == 13) {  // exactly 2^27: legal, incomplete
    put_varint(b, (uint64_t)1 << 27);
    b.insert(b.end(), below(40), 0x11);
  } else if (cls == 14) {  // 2^27 + 1: error
    put_varint(b, ((uint64_t)1 << 27) + 1);
    b.insert(b.end(), below(40), 0x11);
  } else if (cls == 15) {  // a ten-byte varint whose last byte is 2: > u64
    b.insert(b.end(), 9, 0xFF);
    b.push_back(0x02);
  } else if (cls == 16) {  // a body cut short
    const uint64_t len = 2 + pick_len(true);
    put_varint(b, len);
    b.insert(b.end(), (size_t)below(len), 0x7B);
  } else if (cls == 17) {  // a two- or three-byte varint cut inside
    Bytes h;
    put_varint(h, below(2) ? 300 : 70000);
    b.insert(b.end(), h.begin(), h.end() - 1 - below(h.size() - 1));
  }
}

static Segment make_segment(uint32_t T_edge, bool long_ok) {
  Bytes b;
  const bool zero_run = below(12) == 0;
  const uint64_t n = zero_run ? 1000 + below(300) : below(30) == 0 ? 300 + below(200) : below(40);
  for (uint64_t i = 0; i < n; ++i) put_frame(b, zero_run ? (below(50) ? 0 : 1) : pick_len(long_ok && below(2) == 0));
  const int cls = (int)below(N_TAILS + 4);
  if (cls < N_TAILS) {
    if (below(3) == 0 && cls != 0) {  // the stop or error lands on a tile edge: its varint starts on the last byte
      const uint64_t want = ((b.size() + T_edge) & ~(uint64_t)(T_edge - 1)) - 1 - below(2);  // edge - 1 or edge - 2
      while (b.size() + 400 < want) put_frame(b, 336 + below(44));
      if (want > b.size()) {
        const uint64_t gap = want - b.size();  // one frame of exactly gap bytes
        if (gap != 129) put_frame(b, gap <= 128 ? gap - 1 : gap - 2);  // (gap <= 400: a one- or two-byte varint)
      }
      ++n_tile_edge_err;
    }
    put_tail(b, cls);
    ++n_tail_seen[cls];
    if (below(2)) {  // mid-stream: frames behind it, which no index may report after an error or a stop
      for (uint64_t i = 0; i < 5; ++i) put_frame(b, pick_len(false));
      ++n_stop_mid;
    }
  } else if (cls == N_TAILS && !b.empty()) {  // a cut at a random byte: inside a varint, a body, or on a boundary
    b.resize(below(b.size() + 1));
  }
  Segment sg;
  sg.len = b.size();
  sg.buf.reset(new uint8_t[b.size()]);
  if (!b.empty()) memcpy(sg.buf.get(), b.data(), b.size());
  sg.peer = (uint16_t)below(65535);
  return sg;
}

static size_t n_streams, n_segments, n_frames_total, n_outside, n_capped, n_long_entry;

// below_total: frame_cap is drawn below the number of frames; else above it
static void check_case(std::vector<Segment>& segs, uint64_t stream_bytes, bool below_total,
                       const std::vector<uint32_t>& tiles) {
  // the oracle, per segment
  std::vector<uint64_t> exp_off;
  std::vector<uint32_t> exp_len;
  std::vector<uint16_t> exp_peer;
  std::vector<ix_head> exp_heads(segs.size());
  uint64_t run = 0;
  for (size_t s = 0; s < segs.size(); ++s) {
    Segment& sg = segs[s];
    ix_head& h = exp_heads[s];
    memset(&h, 0, sizeof h);
    h.first = (uint32_t)exp_off.size();
    bool in = sg.inside;
    if (in) {
      run += sg.len;
      in = run <= stream_bytes;
    }
    if (!in) {
      h.status = PBFT_SEG_EOUTSIDE;
      ++n_outside;
      continue;
    }
    std::vector<uint64_t> off(sg.len + 1);
    std::vector<uint32_t> flen(sg.len + 1);
    uint64_t nf = 0, used = 0;
    const int rc = pbft_wire_frame_index(sg.buf.get(), sg.len, sg.len + 1, off.data(), flen.data(), &nf, &used);
    CHECK(rc == 0 || rc == PBFT_EINVAL);
    h.status = rc ? PBFT_SEG_EFRAMING : PBFT_SEG_OK;
    n_err += rc ? 1 : 0;
    h.n_frames = (uint32_t)nf;
    h.consumed = used;
    for (uint64_t f = 0; f < nf; ++f) {
      exp_off.push_back(sg.off + off[f]);
      exp_len.push_back(flen[f]);
      exp_peer.push_back(sg.peer);
      if (flen[f] > 400) ++n_long_entry;
    }
  }
  const uint64_t total = exp_off.size();
  const uint64_t frame_cap = below_total ? below(total + 1) : total + below(300);
  n_frames_total += total;
  n_segments += segs.size();
  if (frame_cap < total) ++n_capped;
  for (uint32_t T : tiles) {
    const Index got = host_index(segs, stream_bytes, T, frame_cap);
    CHECK(got.n_frames[0] == total);
    CHECK(got.n_frames[1] == (total > frame_cap ? total - frame_cap : 0));
    for (size_t s = 0; s < segs.size(); ++s) {
      const ix_head &g = got.heads[s], &e = exp_heads[s];
      CHECK(g.status == e.status);
      CHECK(g.n_frames == e.n_frames);
      CHECK(g.consumed == e.consumed);
      CHECK(g.first == e.first && g.pad == 0);
    }
    for (uint64_t f = 0; f < frame_cap; ++f) {
      if (f < total) CHECK(got.off[f] == exp_off[f] && got.len[f] == exp_len[f] && got.peer[f] == exp_peer[f]);
      else CHECK(got.off[f] == 0 && got.len[f] == 0 && got.peer[f] == 0xFFFF);
    }
  }
}

int main() {
  static_assert(sizeof(ix_head) == sizeof(pbft_seg_head), "the core's head is the header's");
  static_assert(IX_STOP - 1 == PBFT_SEG_OK && IX_ERR - 1 == PBFT_SEG_EFRAMING && IX_SEG_OUTSIDE == PBFT_SEG_EOUTSIDE,
                "the core's status values are the header's");
  static_assert(IX_UVI_MAX_FRAME == PBFT_UVI_MAX_FRAME, "the core's frame limit is the header's");
  const std::vector<uint32_t> both = {IX_TILE_MIN, IX_TILE_MAX}, all = {IX_TILE_MIN, 2048, IX_TILE_MAX};
  for (int it = 0; it < 2200; ++it) {
    std::vector<Segment> segs;
    const uint32_t S = it % 7 == 0 ? 1 + (uint32_t)below(9) : 1;
    uint64_t at = 0;
    for (uint32_t s = 0; s < S; ++s) {
      segs.push_back(make_segment(it % 5 == 4 ? IX_TILE_MAX : IX_TILE_MIN, it % 10 == 9));
      at += below(40);  // gaps, any alignment
      segs.back().off = at;
      at += segs.back().len;
    }
    uint64_t stream_bytes = at + below(20);
    if (S > 2 && below(3) == 0) segs[1].off = stream_bytes - segs[1].len / 2 + 1;  // it ends behind the stream
    if (S > 3 && below(3) == 0) segs[2].off = segs[0].off;  // overlap: the lengths may add up to more than the stream
    if (S > 3 && below(4) == 0) stream_bytes = at - segs.back().len / 2;
    for (Segment& sg : segs) sg.inside = sg.off + sg.len <= stream_bytes;
    check_case(segs, stream_bytes, it % 6 == 0, it % 50 == 0 ? all : both);
    ++n_streams;
  }
  // fixed shapes: empty input, no segment, a run of 1,000 zero-length frames, one 70,000-byte frame between votes
  {
    std::vector<Segment> none;
    check_case(none, 0, false, both);
    std::vector<Segment> segs(3);
    for (Segment& sg : segs) sg.buf.reset(new uint8_t[0]);
    check_case(segs, 0, false, both);
    Bytes b;
    for (int i = 0; i < 1000; ++i) put_frame(b, 0);
    put_frame(b, 350);
    put_frame(b, 70000);
    put_frame(b, 1100);  // (a PrePrepare's size: the next entry is >= IX_ENTRIES)
    put_frame(b, 350);
    b.push_back(0xD4);  // a varint cut by the segment's end
    std::vector<Segment> one(1);
    one[0].len = b.size();
    one[0].buf.reset(new uint8_t[b.size()]);
    memcpy(one[0].buf.get(), b.data(), b.size());
    one[0].off = 13;
    check_case(one, b.size() + 13, false, all);
    check_case(one, b.size() + 13, true, all);
    n_streams += 3;
  }
  for (int c = 1; c < N_TAILS; ++c) CHECK(n_tail_seen[c] >= 20);
  CHECK(n_err >= 200 && n_stop_mid >= 200 && n_tile_edge_err >= 100 && n_outside >= 20 && n_capped >= 100);
  CHECK(n_long_entry >= 200);
  printf("indexed streams: %zu (%zu segments, %zu frames)\n", n_streams, n_segments, n_frames_total);
  printf("framing errors: %zu, stops with frames behind: %zu, on a tile edge: %zu, outside: %zu, capped: %zu\n", n_err,
         n_stop_mid, n_tile_edge_err, n_outside, n_capped);
  printf("index host run ok\n");
  return 0;
}
