// TEST INFRASTRUCTURE: pbft_replica_push_streams against the sequence it is defined by, in C++ under AddressSanitizer
// + UndefinedBehaviorSanitizer (built and run by tests/test_replica_streams.py, host only).  Two replicas of
// one 7-replica network get the same random traffic, call after call (a fixed seed): replica A through a forced
// flush, pbft_replica_push_frames per segment and a forced flush; replica B through pbft_replica_push_streams, whose
// front half runs on the host under a verifier override -- here a fake one whose answer is a function of the signature
// bytes, so "forged" is one bit of the frame.  After every call: the same consumed per segment, pushed, dropped, sorted
// events, counters and predicates.  Now and then the caps are set low, so the whole-call fallback runs here too.
// The replica is linked without the GPU library: the few verifier entry points it names are stubs that report no device.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/pbft_replica.h"
#include "../../include/pbft_wire.h"

#define CHECK(c)                                                             \
  do {                                                                       \
    if (!(c)) {                                                              \
      fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); \
      exit(1);                                                               \
    }                                                                        \
  } while (0)

// ---- what replica.cpp links against from the GPU library: never reached without a context ----
extern "C" {
#define NODEV(name, ...) \
  int name(__VA_ARGS__) { return PBFT_ENODEV; }
NODEV(pbft_verify_ctx_clone, pbft_ctx*, pbft_ctx**)
NODEV(pbft_verify_ctx_destroy, pbft_ctx*)
NODEV(pbft_digest_blake2b512, pbft_ctx*, const uint8_t*, const uint64_t*, const uint32_t*, uint64_t, uint8_t*)
NODEV(pbft_verify_votes_stage, pbft_ctx*, uint64_t, uint32_t, pbft_votes_staging*)
NODEV(pbft_verify_votes_submit, pbft_ctx*, uint64_t, uint32_t, uint64_t*)
NODEV(pbft_verify_votes_submit_begin, pbft_ctx*, uint64_t, uint32_t, uint64_t*)
NODEV(pbft_verify_votes_submit_rows, pbft_ctx*, uint64_t)
NODEV(pbft_verify_votes_submit_host, pbft_ctx*, const uint8_t*, uint64_t, const uint8_t*, uint32_t, uint64_t*)
NODEV(pbft_verify_votes_open, pbft_ctx*, uint64_t, uint32_t, uint64_t*)
NODEV(pbft_verify_votes_piece, pbft_ctx*, const uint8_t*, uint64_t, uint64_t, const uint8_t*, uint32_t, uint32_t)
NODEV(pbft_verify_votes_close, pbft_ctx*, uint64_t)
NODEV(pbft_verify_poll_rows, pbft_ctx*, uint64_t*)
NODEV(pbft_verify_poll, pbft_ctx*)
NODEV(pbft_verify_wait, pbft_ctx*)
NODEV(pbft_verify_update_keys, pbft_ctx*, const uint32_t*, const uint8_t*, uint32_t, uint8_t*)
NODEV(pbft_verify_revoke_keys, pbft_ctx*, const uint32_t*, uint32_t)
NODEV(pbft_verify_key_set_id, pbft_ctx*, uint64_t*)
NODEV(pbft_host_alloc, pbft_ctx*, size_t, void**)
NODEV(pbft_host_free, pbft_ctx*, void*)
}

static const uint32_t N_REP = 7, WINDOW = 8;
static const uint64_t VIEW = 1;
static std::mt19937_64 rng(20261020);
static uint64_t below(uint64_t n) { return rng() % n; }

// valid iff the signature's first byte is even
static int fake_verify(void*, const uint8_t* R, const uint8_t*, const uint16_t*, const uint8_t*, uint32_t, uint32_t,
                       uint64_t N, uint64_t* out) {
  for (uint64_t w = 0; w < (N + 63) / 64; ++w) out[w] = 0;
  for (uint64_t i = 0; i < N; ++i)
    if (!(R[32 * i] & 1)) out[i >> 6] |= (uint64_t)1 << (i & 63);
  return 0;
}
// 64 bytes spread from an FNV-1a of the operation
static void fake_digest_of(const uint8_t* op, uint32_t n, uint8_t out[64]) {
  uint64_t x = 1469598103934665603ull;
  for (uint32_t i = 0; i < n; ++i) x = (x ^ op[i]) * 1099511628211ull;
  for (int i = 0; i < 64; ++i) {
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    out[i] = (uint8_t)(x >> 56);
  }
}
static int fake_digest(void*, const uint8_t* op, uint32_t n, uint8_t out[64]) {
  fake_digest_of(op, n, out);
  return 0;
}

static pbft_replica* make_replica() {
  std::vector<uint8_t> keys(32 * N_REP);
  for (size_t i = 0; i < keys.size(); ++i) keys[i] = (uint8_t)(i * 37 + i / 32);
  pbft_replica* r = nullptr;
  CHECK(pbft_replica_create(nullptr, N_REP, 0, keys.data(), &r) == 0);
  CHECK(pbft_replica_set_verifier(r, fake_verify, nullptr) == 0);
  CHECK(pbft_replica_set_digest_fn(r, fake_digest, nullptr) == 0);
  CHECK(pbft_replica_set_log_window(r, WINDOW) == 0);
  return r;
}

static std::string op_of(uint64_t seq, int variant) { return "op-" + std::to_string(seq) + (variant ? "-x" : ""); }

static void append_frame(std::vector<uint8_t>& out, const pbft_wire_msg& m) {
  uint8_t buf[2048];
  size_t len = 0;
  CHECK(pbft_wire_encode_frame(&m, buf, sizeof buf, &len) == 0);
  out.insert(out.end(), buf, buf + len);
}
static void append_raw(std::vector<uint8_t>& out, const std::string& body) {
  uint8_t v[10];
  const size_t hn = pbft_uvi_encode(body.size(), v);
  out.insert(out.end(), v, v + hn);
  out.insert(out.end(), body.begin(), body.end());
}

// One random frame from `peer`'s connection around sequence number `base`.
static void random_frame(std::vector<uint8_t>& out, uint32_t peer, uint64_t base) {
  const uint64_t x = below(100);
  pbft_wire_msg m;
  memset(&m, 0, sizeof m);
  const uint64_t seq = x < 80 ? base + below(4) : x < 90 ? base + below(WINDOW + 4) : below(3) ? base - 1 - below(2) : ~0ull;
  const int variant = below(8) == 0;
  const std::string op = op_of(seq, variant);
  m.view = below(25) ? VIEW : below(3);
  m.seq = seq;
  fake_digest_of((const uint8_t*)op.data(), (uint32_t)op.size(), m.digest);
  m.digest_ok = 1;
  m.has_sig = 1;
  m.replica = below(20) ? peer : (uint32_t)below(N_REP + 2);
  for (int i = 0; i < 64; ++i) m.sig[i] = (uint8_t)rng();
  m.sig[0] = (uint8_t)((m.sig[0] & ~1u) | (below(6) == 0));  // one in six is forged
  if (x >= 97) {
    append_raw(out, below(2) ? "{\"ClientRequest\":{\"operation\":\"x\",\"timestamp\":1,\"client\":\"127.0.0.1:80\"}}" : "junk");
    return;
  }
  if (x >= 92 || (peer == VIEW % N_REP && below(4) == 0)) {
    m.kind = PBFT_MSG_PREPREPARE;
    m.operation = op.data();
    m.operation_len = (uint32_t)op.size();
    m.timestamp = 7;
    snprintf(m.client, sizeof m.client, "127.0.0.1:8080");
    if (below(3)) m.replica = (uint32_t)(VIEW % N_REP);
    append_frame(out, m);
    return;
  }
  m.kind = below(2) ? PBFT_MSG_PREPARE : PBFT_MSG_COMMIT;
  const size_t at = out.size();
  append_frame(out, m);
  if (below(6) == 0) {  // the same vote again, the same vote with another signature, or another digest: contested rows
    const int how = (int)below(3);
    if (how == 1) m.sig[5] ^= 0x10;
    if (how == 2) m.digest[0] ^= 1;
    append_frame(out, m);
  }
  if (below(40) == 0) {  // not canonical, still this vote: a space behind the first colon
    std::vector<uint8_t> f(out.begin() + at, out.end());
    out.resize(at);
    size_t hn = 0;
    uint64_t fl = 0;
    CHECK(pbft_uvi_decode(f.data(), f.size(), &fl, &hn) == 0);
    std::string body((const char*)f.data() + hn, (size_t)fl);
    body.insert(body.find(':') + 1, " ");
    append_raw(out, body);
    out.insert(out.end(), f.begin() + hn + (size_t)fl, f.end());
  }
}

// What a correct replica sends in a round: the primary its PrePrepare, everybody a Prepare and a Commit (one signature
// in eight forged).
static void honest_frames(std::vector<uint8_t>& out, uint32_t peer, uint64_t seq) {
  const std::string op = op_of(seq, 0);
  for (uint32_t kind = peer == VIEW % N_REP ? 0 : 1; kind <= 2; ++kind) {
    pbft_wire_msg m;
    memset(&m, 0, sizeof m);
    m.kind = kind;
    m.view = VIEW;
    m.seq = seq;
    fake_digest_of((const uint8_t*)op.data(), (uint32_t)op.size(), m.digest);
    m.digest_ok = m.has_sig = 1;
    m.replica = peer;
    for (int i = 0; i < 64; ++i) m.sig[i] = (uint8_t)rng();
    m.sig[0] = (uint8_t)((m.sig[0] & ~1u) | (below(8) == 0));
    if (kind == 0) {
      m.operation = op.data();
      m.operation_len = (uint32_t)op.size();
      m.timestamp = 7;
      snprintf(m.client, sizeof m.client, "127.0.0.1:8080");
    }
    append_frame(out, m);
  }
}

struct Outcome {
  std::vector<uint64_t> consumed;
  std::vector<uint32_t> status;
  uint64_t pushed = 0, dropped = 0;
  std::vector<std::tuple<uint64_t, uint64_t, uint32_t>> events;
};

static void flush_into(pbft_replica* r, Outcome& o) {
  std::vector<pbft_round_event> ev(4096);
  uint32_t ne = 0;
  CHECK(pbft_replica_flush(r, 1, ev.data(), (uint32_t)ev.size(), &ne) == 0);
  for (uint32_t i = 0; i < ne; ++i) o.events.emplace_back(ev[i].view, ev[i].seq, ev[i].kind);
}

static void same_state(pbft_replica* a, pbft_replica* b, uint64_t hi) {
  pbft_replica_stats x, y;
  CHECK(pbft_replica_get_stats(a, &x) == 0 && pbft_replica_get_stats(b, &y) == 0);
  CHECK(x.accepted == y.accepted && x.rejected_sig == y.rejected_sig && x.rejected_digest == y.rejected_digest);
  CHECK(x.rejected_view == y.rejected_view && x.rejected_watermark == y.rejected_watermark);
  CHECK(x.rejected_signer == y.rejected_signer && x.duplicates == y.duplicates && x.dropped_flood == y.dropped_flood);
  CHECK(x.windows_gc == y.windows_gc && x.low_watermark == y.low_watermark && x.live_windows == y.live_windows);
  for (uint64_t v = 0; v < 3; ++v)
    for (uint64_t q = 0; q <= hi; ++q) {
      CHECK(pbft_replica_prepared(a, v, q) == pbft_replica_prepared(b, v, q));
      CHECK(pbft_replica_committed_local(a, v, q) == pbft_replica_committed_local(b, v, q));
    }
}

int main() {
  pbft_replica *A = make_replica(), *B = make_replica();
  const int CALLS = 400;
  uint64_t frames_bytes = 0, segments = 0, n_events = 0;
  for (int call = 0; call < CALLS; ++call) {
    pbft_replica_stats now;
    CHECK(pbft_replica_get_stats(A, &now) == 0);
    const uint64_t base = now.low_watermark + 1;  // the rounds move on as windows commit and are collected
    const uint32_t S = (uint32_t)below(9);
    std::vector<uint8_t> stream;
    std::vector<uint64_t> off, len;
    std::vector<uint16_t> peer;
    for (uint32_t s = 0; s < S; ++s) {
      std::vector<uint8_t> seg;
      const uint32_t p = (uint32_t)below(N_REP);
      const uint32_t k = (uint32_t)below(14);
      const uint32_t junk_at = below(25) == 0 ? (uint32_t)below(k + 1) : ~0u;
      if (below(10) < 7)
        for (uint64_t q = base; q < base + 2; ++q) honest_frames(seg, p, q);
      for (uint32_t f = 0; f < k; ++f) {
        if (f == junk_at) seg.insert(seg.end(), 11, 0xFF);  // an overlong varint: a framing error
        random_frame(seg, p, base);
      }
      if (below(4) == 0 && !seg.empty()) seg.resize(seg.size() - 1 - below(std::min<size_t>(seg.size(), 420)));
      stream.insert(stream.end(), 1 + below(7), 0x7B);  // a gap
      off.push_back(stream.size());
      len.push_back(seg.size());
      peer.push_back((uint16_t)p);
      stream.insert(stream.end(), seg.begin(), seg.end());
      frames_bytes += seg.size();
    }
    segments += S;
    // the stream in a heap buffer of exactly its length: a read past it is a heap overflow
    std::vector<uint8_t> exact(stream);
    exact.shrink_to_fit();
    Outcome want, got;
    flush_into(A, want);
    for (uint32_t s = 0; s < S; ++s) {
      uint64_t used = 0, np = 0, nd = 0;
      const int rc = pbft_replica_push_frames(A, peer[s], exact.data() + off[s], (size_t)len[s], &used, &np, &nd);
      CHECK(rc == 0 || rc == PBFT_EINVAL);
      want.consumed.push_back(used);
      want.status.push_back(rc ? PBFT_SEG_EFRAMING : PBFT_SEG_OK);
      want.pushed += np;
      want.dropped += nd;
    }
    flush_into(A, want);
    std::sort(want.events.begin(), want.events.end());
    const bool low_caps = call % 23 == 7;
    CHECK(pbft_replica_reserve_streams(B, 0, 0, low_caps ? 2 : 1 << 16, low_caps ? 1 : 1 << 12, low_caps ? 0 : 1 << 12) == 0);
    std::vector<pbft_seg_head> heads(S + 1);
    std::vector<pbft_round_event> ev(4096);
    uint32_t ne = 0;
    CHECK(pbft_replica_push_streams(B, exact.data(), exact.size(), off.data(), len.data(), peer.data(), S, heads.data(),
                                    &got.pushed, &got.dropped, ev.data(), (uint32_t)ev.size(), &ne) == 0);
    for (uint32_t i = 0; i < ne; ++i) got.events.emplace_back(ev[i].view, ev[i].seq, ev[i].kind);
    CHECK(std::is_sorted(got.events.begin(), got.events.end()));
    uint32_t first = 0;
    for (uint32_t s = 0; s < S; ++s) {
      got.consumed.push_back(heads[s].consumed);
      got.status.push_back(heads[s].status);
      CHECK(heads[s].first == first && heads[s].pad == 0);
      first += heads[s].n_frames;
    }
    CHECK(got.consumed == want.consumed && got.status == want.status);
    if (got.pushed != want.pushed || got.dropped != want.dropped)
      fprintf(stderr, "call %d (%u segments): pushed %llu, the host sequence %llu; dropped %llu, the host sequence %llu\n",
              call, S, (unsigned long long)got.pushed, (unsigned long long)want.pushed,
              (unsigned long long)got.dropped, (unsigned long long)want.dropped);
    CHECK(got.pushed == want.pushed && got.dropped == want.dropped);
    CHECK(got.events == want.events);
    same_state(A, B, base + WINDOW + 6);
    n_events += ne;
  }
  pbft_replica_stats st;
  pbft_replica_streams_stats ss;
  CHECK(pbft_replica_get_stats(B, &st) == 0 && pbft_replica_get_streams_stats(B, &ss) == 0);
  printf("streams host run ok: %d calls, %llu segments, %llu bytes, %llu events, %llu clean, %llu residue, "
         "%llu fallbacks\n",
         CALLS, (unsigned long long)segments, (unsigned long long)frames_bytes, (unsigned long long)n_events,
         (unsigned long long)ss.clean_rows, (unsigned long long)ss.residue_rows,
         (unsigned long long)(ss.fallback_frames + ss.fallback_envelopes + ss.fallback_residue + ss.fallback_deferred));
  printf("counters: accepted %llu, rejected_sig %llu, rejected_digest %llu, rejected_view %llu, rejected_watermark "
         "%llu, rejected_signer %llu, duplicates %llu, dropped_flood %llu, windows_gc %llu, host-front calls %llu\n",
         (unsigned long long)st.accepted, (unsigned long long)st.rejected_sig, (unsigned long long)st.rejected_digest,
         (unsigned long long)st.rejected_view, (unsigned long long)st.rejected_watermark,
         (unsigned long long)st.rejected_signer, (unsigned long long)st.duplicates,
         (unsigned long long)st.dropped_flood, (unsigned long long)st.windows_gc,
         (unsigned long long)ss.calls_host_front);
  // the traffic reached what it is there for: every counter moved, rounds committed and were collected, both the
  // signer sets and the residue carried votes, and the whole-call fallback ran for a cap and for a deferred twin
  CHECK(ss.calls_device == 0 && ss.calls_host_front > 0 && ss.clean_rows > 0 && ss.residue_rows > 0);
  CHECK(st.accepted && st.rejected_sig && st.rejected_digest && st.rejected_view && st.rejected_watermark);
  CHECK(st.rejected_signer && st.duplicates && st.dropped_flood && st.windows_gc && st.low_watermark);
  CHECK(ss.fallback_frames + ss.fallback_envelopes + ss.fallback_residue > 0 && ss.fallback_deferred > 0);
  CHECK(pbft_replica_destroy(A) == 0 && pbft_replica_destroy(B) == 0);
  return 0;
}
