// TEST INFRASTRUCTURE: the host build of the frame decoder's parse core (pbft_amd/csrc/wire_decode_core.h, the code
// each GPU lane runs in wire_decode.hip) under AddressSanitizer + UndefinedBehaviorSanitizer, against the host's own
// parser (wire.cpp).  Built and run by tests/test_frames.py, host only.  Every frame the core sees lies in a heap
// buffer of exactly its length, so any read outside it is a heap overflow; the row around the frame (the bytes an LDS
// row would hold past the frame) is presented with several fillers and start positions, which must not matter.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../include/pbft_replica.h"
#include "../../include/pbft_wire.h"
#include "../../pbft_amd/csrc/wire_decode_core.h"

using namespace pbft;

#define CHECK(c)                                                             \
  do {                                                                       \
    if (!(c)) {                                                              \
      fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); \
      exit(1);                                                               \
    }                                                                        \
  } while (0)

// wire.cpp's pbft_wire_decode_votes needs it; the layout as include/pbft_replica.h documents it
extern "C" void pbft_envelope(uint8_t out[PBFT_ENVELOPE_BYTES], uint8_t kind, uint64_t view, uint64_t seq,
                              const uint8_t digest[64]) {
  memcpy(out, "PBFT", 4);
  out[4] = kind;
  for (int i = 0; i < 8; ++i) out[5 + i] = (uint8_t)(view >> (8 * i));
  for (int i = 0; i < 8; ++i) out[13 + i] = (uint8_t)(seq >> (8 * i));
  memcpy(out + 21, digest, 64);
}

typedef std::string Bytes;  // (a frame body; copied into an exactly-sized heap buffer before anything parses it)

static std::mt19937_64 rng(20261019);

static Bytes encode(const pbft_wire_msg& m, bool with_varint = false) {
  size_t n = 0;
  pbft_wire_encode_frame(&m, nullptr, 0, &n);
  CHECK(n > 0);
  std::vector<uint8_t> buf(n);
  CHECK(pbft_wire_encode_frame(&m, buf.data(), n, &n) == 0);
  if (with_varint) return Bytes((const char*)buf.data(), n);
  uint64_t fl;
  size_t hn;
  CHECK(pbft_uvi_decode(buf.data(), n, &fl, &hn) == 0 && hn + fl == n);
  return Bytes((const char*)buf.data() + hn, (size_t)fl);
}

static pbft_wire_msg vote(uint32_t kind, uint64_t view, uint64_t seq, uint32_t replica, bool sign = true) {
  pbft_wire_msg m;
  memset(&m, 0, sizeof m);
  m.kind = kind;
  m.view = view;
  m.seq = seq;
  for (int i = 0; i < 64; ++i) m.digest[i] = (uint8_t)rng();
  m.digest_ok = 1;
  m.has_sig = sign ? 1 : 0;
  m.replica = replica;
  for (int i = 0; i < 64; ++i) m.sig[i] = (uint8_t)rng();
  m.operation = "";
  return m;
}

struct Core {
  uint32_t status;
  uint32_t rec[40];
  frame_fields h;
};

static Core run_core_at(const Bytes& body, uint32_t n_replicas, uint32_t peer, uint32_t b0, uint8_t fill) {
  std::unique_ptr<uint8_t[]> exact(new uint8_t[body.size()]);
  memcpy(exact.get(), body.data(), body.size());
  Core c;
  const frame_mem_reader rd{exact.get(), b0, (uint32_t)body.size(), fill};
  c.status = wire_decode_frame(rd, b0, (uint32_t)body.size(), n_replicas, peer, c.rec, c.h);
  CHECK(c.status == c.h.status);
  return c;
}

// the same answer wherever the frame starts in its row and whatever surrounds it
static Core run_core(const Bytes& body, uint32_t n_replicas, uint32_t peer) {
  static const uint8_t FILL[6] = {0x00, 0xAA, '0', 'a', '"', '}'};
  static unsigned turn = 0;
  const Core c = run_core_at(body, n_replicas, peer, 0, 0);
  ++turn;
  const Core d = run_core_at(body, n_replicas, peer, turn & 3, FILL[turn % 6]);
  CHECK(c.status == d.status && memcmp(c.rec, d.rec, sizeof c.rec) == 0);
  CHECK(c.h.view == d.h.view && c.h.seq == d.h.seq && c.h.kind == d.h.kind && c.h.key_idx == d.h.key_idx);
  return c;
}

struct Host {
  bool ok;
  pbft_wire_msg m;
};

static Host run_host(const Bytes& body) {
  std::unique_ptr<char[]> exact(new char[body.size() + 1]);  // (+1: never an empty allocation handed to the parser)
  memcpy(exact.get(), body.data(), body.size());
  static char arena[1 << 16];
  Host h;
  h.ok = pbft_wire_decode_json(exact.get(), body.size(), &h.m, arena, sizeof arena) == 0;
  return h;
}

static void check_zero(const Core& c) {
  for (int k = 0; k < 40; ++k) CHECK(c.rec[k] == (k == 37 ? 0xFFFF0000u : 0u));
  CHECK(c.h.view == 0 && c.h.seq == 0 && c.h.kind == 0 && c.h.key_idx == 0xFFFF);
}

static void check_ok(const Core& c, const pbft_wire_msg& m) {
  uint8_t env[PBFT_ENVELOPE_BYTES], want[PBFT_RECORD_BYTES];
  pbft_envelope(env, (uint8_t)m.kind, m.view, m.seq, m.digest);
  const uint16_t k = (uint16_t)m.replica;
  CHECK(pbft_records_pack(m.sig, m.sig + 32, &k, env, PBFT_ENVELOPE_BYTES, 1, want) == 0);
  CHECK(memcmp(c.rec, want, PBFT_RECORD_BYTES) == 0);  // (x86-64: the words in memory are the record's bytes)
  CHECK(c.h.view == m.view && c.h.seq == m.seq && c.h.kind == m.kind && c.h.key_idx == m.replica);
}

static uint64_t random_width_u64() {  // every decimal width 1..20
  const int bits = (int)(rng() % 65);
  return bits == 0 ? 0 : rng() >> (64 - bits);
}

static uint64_t n_canonical = 0, n_mutated = 0, n_mut_accepted = 0, n_mut_host_ok = 0;

static void canonical() {
  const uint64_t NUMS[7] = {0, 9, 10, 99, 1ull << 32, 10000000000000000000ull, ~0ull};
  const uint32_t REPS[6] = {0, 9, 10, 255, 256, 65535};
  const uint32_t NREP[5] = {1, 10, 256, 257, 65535};
  bool len_seen[FRAME_MAX + 1] = {};
  auto one = [&](uint32_t kind, uint64_t view, uint64_t seq, uint32_t rep) {
    const pbft_wire_msg m = vote(kind, view, seq, rep);
    const Bytes body = encode(m);
    CHECK(body.size() >= FRAME_MIN && body.size() <= FRAME_MAX);
    len_seen[body.size()] = true;
    const uint32_t n_rep = NREP[rng() % 5];
    const uint32_t pick = (uint32_t)(rng() % 3);
    const uint32_t peer = pick == 0 ? FRAME_NO_PEER : pick == 1 ? rep : REPS[rng() % 6];
    const Core c = run_core(body, n_rep, peer);
    CHECK(c.status != WIRE_ST_EDEFER);
    const bool esigner = rep >= n_rep || (peer != FRAME_NO_PEER && rep != peer);
    CHECK((c.status == WIRE_ST_ESIGNER) == esigner);
    const Host h = run_host(body);
    CHECK(h.ok && h.m.kind == kind && h.m.has_sig && h.m.digest_ok);
    if (c.status == WIRE_ST_OK) check_ok(c, h.m);
    else check_zero(c);
    ++n_canonical;
  };
  for (uint32_t kind = 1; kind <= 2; ++kind)
    for (uint64_t v : NUMS)
      for (uint64_t s : NUMS)
        for (uint32_t r : REPS) one(kind, v, s, r);
  while (n_canonical < 24000) {
    const uint32_t rep = rng() % 4 ? REPS[rng() % 6] : (uint32_t)(rng() % 65536);
    one(1 + (uint32_t)(rng() % 2), rng() % 3 ? random_width_u64() : NUMS[rng() % 7],
        rng() % 3 ? random_width_u64() : NUMS[rng() % 7], rep);
  }
  CHECK(len_seen[FRAME_MIN] && len_seen[FRAME_MAX]);
}

// Exact agreement with the host's rule.  A body is canonical iff the general parser reads a signed Prepare / Commit
// from it AND writing that message back gives the same bytes; the core must accept exactly those.
static void mutant(const Bytes& body) {
  const Core c = run_core(body, 65535, FRAME_NO_PEER);
  const Host h = run_host(body);
  bool canon = false;
  if (h.ok && (h.m.kind == PBFT_MSG_PREPARE || h.m.kind == PBFT_MSG_COMMIT) && h.m.has_sig && h.m.digest_ok)
    canon = encode(h.m) == body;
  if (c.status == WIRE_ST_EDEFER) {
    CHECK(!canon);
    check_zero(c);
  } else {
    CHECK(canon);
    if (h.m.replica == 65535) {
      CHECK(c.status == WIRE_ST_ESIGNER);
      check_zero(c);
    } else {
      CHECK(c.status == WIRE_ST_OK);
      check_ok(c, h.m);
    }
    ++n_mut_accepted;
  }
  n_mut_host_ok += h.ok;
  ++n_mutated;
}

static Bytes replaced(Bytes s, const char* what, const char* with) {
  const size_t at = s.find(what);
  CHECK(at != Bytes::npos);
  return s.replace(at, strlen(what), with);
}

static void mutations() {
  std::vector<Bytes> bases;
  bases.push_back(encode(vote(PBFT_MSG_COMMIT, 1, 2, 3)));                                   // 336
  bases.push_back(encode(vote(PBFT_MSG_PREPARE, ~0ull, 10000000000000000000ull, 65534)));    // 379
  for (int i = 0; i < 10; ++i)
    bases.push_back(encode(vote(1 + (uint32_t)(rng() % 2), random_width_u64(), random_width_u64(),
                                (uint32_t)(rng() % 65535))));
  const char INS[8] = {' ', '0', '1', 'a', '"', ',', '}', '\\'};
  for (const Bytes& b : bases) {
    mutant(b);
    for (size_t i = 0; i < b.size(); ++i) {  // every position: a bit flip, a replaced, an inserted and a deleted byte
      Bytes m = b;
      m[i] = (char)(m[i] ^ (1 << (rng() % 8)));
      mutant(m);
      m = b;
      m[i] = INS[rng() % 8];
      mutant(m);
      m = b;
      m.insert(i, 1, INS[rng() % 8]);
      mutant(m);
      m = b;
      m.erase(i, 1);
      mutant(m);
    }
    for (size_t i = 0; i < b.size(); ++i)  // uppercase hex (and uppercased letters of the skeleton)
      if (b[i] >= 'a' && b[i] <= 'z' && rng() % 4 == 0) {
        Bytes m = b;
        m[i] = (char)(m[i] - 32);
        mutant(m);
      }
  }
  for (int rep = 0; rep < 3; ++rep) {  // truncation to every length 0..380 (the longest base padded), and a longer tail
    const Bytes b = bases[rep];
    for (size_t n = 0; n <= 380; ++n) mutant(n <= b.size() ? b.substr(0, n) : b + Bytes(n - b.size(), "} 0"[rng() % 3]));
  }
  const Bytes b = encode(vote(PBFT_MSG_PREPARE, 7, 42, 5));
  const char* NUMS[] = {"07", "00", "042", "18446744073709551616", "18446744073709551615", "99999999999999999999",
                        "184467440737095516150", "-1", "1.0", "1e3", "+1", "", " 1", "1 ", "0x1", "65536", "65535"};
  for (const char* s : NUMS) {
    mutant(replaced(b, "\"view\":7", (std::string("\"view\":") + s).c_str()));
    mutant(replaced(b, "\"sequence_number\":42", (std::string("\"sequence_number\":") + s).c_str()));
    mutant(replaced(b, "\"replica\":5", (std::string("\"replica\":") + s).c_str()));
  }
  const char* WS[] = {" ", "\t", "\n", "\r", "  "};
  const char* TOK[] = {"{\"Prepare\"", ":{", "\"view\"", ":7", ",\"sequence_number\"", ":42", ",\"digest\"", ":\"",
                       "\",\"replica\"", ":5", ",\"signature\"", "}}"};
  for (const char* w : WS)
    for (const char* t : TOK) {
      mutant(replaced(b, t, (std::string(w) + t).c_str()));
      mutant(replaced(b, t, (std::string(t) + w).c_str()));
    }
  mutant(b + " ");
  mutant(" " + b);
  mutant(b + "\n");
  mutant(b + b);
  // swapped fields, an extra field, a duplicate, an escape in a key: all fine for serde unless duplicated
  {
    const size_t d0 = b.find(",\"digest\""), r0 = b.find(",\"replica\""), s0 = b.find(",\"signature\"");
    const Bytes head = b.substr(0, d0), dg = b.substr(d0, r0 - d0), rp = b.substr(r0, s0 - r0),
                sg = b.substr(s0, b.size() - 2 - s0);
    mutant(head + rp + dg + sg + "}}");
    mutant(head + dg + sg + rp + "}}");
    mutant(head + sg + rp + dg + "}}");
    mutant(head + dg + rp + sg + ",\"x\":1}}");
    mutant(head + ",\"x\":null" + dg + rp + sg + "}}");
    mutant(head + dg + rp + sg + rp + "}}");
    mutant(head + dg + dg + rp + sg + "}}");
    mutant(head + dg + rp + "}}");  // replica without signature
    mutant(head + dg + sg + "}}");
    mutant(replaced(b, "\"view\"", "\"vi\\u0065w\""));
    mutant(replaced(b, "\"Prepare\"", "\"PrePrepare\""));
    mutant(replaced(b, "\"Prepare\"", "\"Commit\""));
    mutant(replaced(b, "\"Prepare\"", "\"prepare\""));
    mutant(replaced(b, "\"Prepare\"", "\"ClientRequest\""));
  }
  mutant(encode(vote(PBFT_MSG_PREPARE, 7, 42, 5, false)));  // unsigned votes
  mutant(encode(vote(PBFT_MSG_COMMIT, 7, 42, 5, false)));
  for (int i = 0; i < 200; ++i) {  // PrePrepares and ClientRequests, some as long as a vote
    pbft_wire_msg m = vote(i & 1 ? PBFT_MSG_PREPREPARE : PBFT_MSG_CLIENT_REQUEST, random_width_u64(),
                           random_width_u64(), (uint32_t)(rng() % 300), (i & 2) != 0);
    const std::string op((size_t)(rng() % 400), 'x');
    m.operation = op.data();
    m.operation_len = (uint32_t)op.size();
    m.timestamp = rng();
    strcpy(m.client, "127.0.0.1:8080");
    mutant(encode(m));
  }
  for (size_t n = 330; n <= 385; ++n) {  // noise of every length around the window, binary and digit runs
    Bytes m(n, 0);
    for (auto& ch : m) ch = (char)rng();
    mutant(m);
    mutant(Bytes("{\"Commit\":{\"view\":") + Bytes(n - 18, '1'));
    mutant(Bytes("{\"Commit\":{\"view\":1,\"sequence_number\":2,\"digest\":\"") + Bytes(n - 50, 'a'));
  }
  while (n_mutated < 52000) {  // several mutations at once
    Bytes m = bases[rng() % bases.size()];
    for (int k = 1 + (int)(rng() % 3); k > 0; --k) {
      const size_t i = rng() % m.size();
      switch (rng() % 3) {
        case 0: m[i] = INS[rng() % 8]; break;
        case 1: m.insert(i, 1, INS[rng() % 8]); break;
        default: m.erase(i, 1);
      }
    }
    mutant(m);
  }
}

// pbft_wire_frame_index against the framing of pbft_wire_decode_votes
static uint64_t n_streams = 0;
static void index_case(const Bytes& stream, uint64_t max_frames) {
  const size_t cap = stream.size() + 1;
  std::unique_ptr<uint8_t[]> exact(new uint8_t[stream.size()]);
  memcpy(exact.get(), stream.data(), stream.size());
  std::vector<uint64_t> off(cap), view(cap), seq(cap);
  std::vector<uint32_t> flen(cap);
  std::vector<uint8_t> status(cap), R(32 * cap), S(32 * cap), msg(PBFT_ENVELOPE_BYTES * cap), kind(cap);
  std::vector<uint16_t> key(cap);
  uint64_t nf = 99, used = 99, nf2 = 99, rows = 99, used2 = 99;
  const int rc = pbft_wire_frame_index(exact.get(), stream.size(), max_frames, off.data(), flen.data(), &nf, &used);
  const int rc2 = pbft_wire_decode_votes(exact.get(), stream.size(), 4, max_frames, cap, status.data(), R.data(),
                                         S.data(), key.data(), msg.data(), kind.data(), view.data(), seq.data(), &nf2,
                                         &rows, &used2);
  CHECK(rc == rc2 && nf == nf2 && used == used2);
  size_t at = 0;
  for (uint64_t f = 0; f < nf; ++f) {  // each body follows its own varint
    uint64_t fl;
    size_t hn;
    CHECK(pbft_uvi_decode(exact.get() + at, stream.size() - at, &fl, &hn) == 0);
    CHECK(off[f] == at + hn && flen[f] == fl);
    at += hn + (size_t)fl;
  }
  CHECK(at == used);
  ++n_streams;
}

static void frame_index() {
  for (int t = 0; t < 60; ++t) {
    Bytes s;
    const int nfr = (int)(rng() % 6);
    for (int i = 0; i < nfr; ++i) {
      switch (rng() % 4) {
        case 0: s += encode(vote(PBFT_MSG_PREPARE, random_width_u64(), random_width_u64(), (uint32_t)(rng() % 6)), true); break;
        case 1: s += encode(vote(PBFT_MSG_COMMIT, 1, 2, 3, false), true); break;
        case 2: s += Bytes("\x03xyz", 4); break;
        default: s += Bytes("\x00", 1);  // an empty frame
      }
    }
    const Bytes whole = encode(vote(PBFT_MSG_COMMIT, 5, 6, 1), true);
    index_case(s, 100);
    index_case(s, 0);
    index_case(s, 2);
    index_case(s + whole.substr(0, 1 + rng() % (whole.size() - 1)), 100);  // an incomplete frame
    index_case(s + Bytes("\x80", 1), 100);                                 // an incomplete varint
    index_case(s + Bytes("\x80\x00", 2) + whole, 100);                     // a non-minimal varint
    index_case(s + Bytes("\x81\x80\x80\x40", 4) + whole, 100);             // 128 MiB + 1: oversized
    index_case(s + Bytes("\xff\xff\xff\xff\xff\xff\xff\xff\xff\x7f", 10), 100);  // > u64
  }
  uint64_t nf, used;
  CHECK(pbft_wire_frame_index(nullptr, 0, 0, nullptr, nullptr, &nf, &used) == 0 && nf == 0 && used == 0);
  CHECK(pbft_wire_frame_index(nullptr, 0, 0, nullptr, nullptr, nullptr, &used) == PBFT_EINVAL);
  CHECK(pbft_wire_frame_index(nullptr, 4, 0, nullptr, nullptr, &nf, &used) == PBFT_EINVAL);
}

int main() {
  static_assert(WIRE_ST_OK == PBFT_WIRE_OK && WIRE_ST_ESIGNER == PBFT_WIRE_ESIGNER && WIRE_ST_EDEFER == PBFT_WIRE_EDEFER, "");
  static_assert(FRAME_MIN == PBFT_FRAME_MIN && FRAME_MAX == PBFT_FRAME_MAX, "");
  static_assert(sizeof(pbft_frame_head) == 24, "");
  canonical();
  mutations();
  frame_index();
  printf("canonical frames: %llu\n", (unsigned long long)n_canonical);
  printf("mutated frames: %llu (%llu canonical, %llu valid for the general parser)\n",
         (unsigned long long)n_mutated, (unsigned long long)n_mut_accepted, (unsigned long long)n_mut_host_ok);
  printf("indexed streams: %llu\n", (unsigned long long)n_streams);
  printf("frames host run ok\n");
  return 0;
}
