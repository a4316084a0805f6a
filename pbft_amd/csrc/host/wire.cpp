// Wire codec of the PBFT messages feeding the GPU verifier (include/pbft_wire.h):
// UviBytes framing (src/protocol_config.rs:41-129) + serde_json encoding of the
// reference's externally tagged Message enum (src/message.rs:7-31), extended
// with the signed-envelope fields "replica" and "signature".
//
// The decoder mirrors serde_json's acceptance rules for these structs: any
// field order and JSON whitespace, unknown fields skipped, duplicate or missing
// fields rejected, u64 numbers without sign / fraction / exponent / leading
// zeros, strings with the JSON escapes (surrogate pairs combined, lone
// surrogates rejected), input must be valid UTF-8 (String::from_utf8 at
// src/message.rs:17).  The reference panics on any of these errors (.unwrap());
// this codec returns PBFT_EINVAL / a per-frame status instead.
#include "../../../include/pbft_wire.h"

#include <stdio.h>
#include <string.h>
#if defined(__SSE2__)
#include <emmintrin.h>
#endif

#include "../../../include/pbft_replica.h"
#include "../propose_core.h"
#include "../reply_core.h"

namespace {

const char HEX[] = "0123456789abcdef";

// ------------------------------------------------------------------ writer
struct Out {
  char* p;
  size_t cap, n = 0;
  void put(char c) {
    if (n < cap) p[n] = c;
    ++n;
  }
  void puts(const char* s) {
    while (*s) put(*s++);
  }
  void u64(uint64_t v) {
    char b[24];
    int k = 0;
    do { b[k++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (k) put(b[--k]);
  }
  void hex(const uint8_t* b, size_t n_) {
    put('"');
    for (size_t i = 0; i < n_; ++i) { put(HEX[b[i] >> 4]); put(HEX[b[i] & 15]); }
    put('"');
  }
  // serde_json string escaping: " \ and control characters (\b \f \n \r \t, else \u00xx)
  void str(const char* s, size_t len) {
    put('"');
    for (size_t i = 0; i < len; ++i) {
      const unsigned char c = (unsigned char)s[i];
      switch (c) {
        case '"': puts("\\\""); break;
        case '\\': puts("\\\\"); break;
        case '\b': puts("\\b"); break;
        case '\f': puts("\\f"); break;
        case '\n': puts("\\n"); break;
        case '\r': puts("\\r"); break;
        case '\t': puts("\\t"); break;
        default:
          if (c < 0x20) { puts("\\u00"); put(HEX[c >> 4]); put(HEX[c & 15]); }
          else put((char)c);
      }
    }
    put('"');
  }
};

void write_client_request(Out& o, const pbft_wire_msg* m) {
  o.puts("{\"operation\":");
  o.str(m->operation ? m->operation : "", m->operation ? m->operation_len : 0);
  o.puts(",\"timestamp\":");
  o.u64(m->timestamp);
  o.puts(",\"client\":");
  o.str(m->client, strnlen(m->client, sizeof m->client));
  o.put('}');
}

// ------------------------------------------------------------------ parser
// (r06: the frames are ASCII but for an operation's text -- 8 bytes per step while no byte has its top bit set)
static inline uint64_t load8(const void* p) {
  uint64_t w;
  memcpy(&w, p, 8);
  return w;
}
bool utf8_valid(const unsigned char* s, size_t n) {
  size_t i = 0;
  while (i < n) {
    while (n - i >= 8 && !(load8(s + i) & 0x8080808080808080ull)) i += 8;
    if (i >= n) break;
    const unsigned char c = s[i];
    if (c < 0x80) { ++i; continue; }
    int k;
    uint32_t cp;
    if ((c & 0xE0) == 0xC0) { k = 1; cp = c & 0x1F; }
    else if ((c & 0xF0) == 0xE0) { k = 2; cp = c & 0x0F; }
    else if ((c & 0xF8) == 0xF0) { k = 3; cp = c & 0x07; }
    else return false;
    if (i + (size_t)k >= n) return false;
    for (int j = 1; j <= k; ++j) {
      if ((s[i + j] & 0xC0) != 0x80) return false;
      cp = (cp << 6) | (s[i + j] & 0x3F);
    }
    if ((k == 1 && cp < 0x80) || (k == 2 && cp < 0x800) || (k == 3 && cp < 0x10000)) return false;  // overlong
    if (cp > 0x10FFFF || (cp >= 0xD800 && cp <= 0xDFFF)) return false;
    i += (size_t)k + 1;
  }
  return true;
}

struct Parser {
  Parser(const char* b, const char* e_, char* a, size_t c) : p(b), e(e_), arena(a), cap(c) {}
  const char* p;
  const char* e;
  char* arena;
  size_t cap, used = 0;

  void ws() {
    while (p < e && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) ++p;
  }
  bool lit(char c) {
    ws();
    if (p < e && *p == c) { ++p; return true; }
    return false;
  }
  bool emit(char c) {
    if (!arena || used >= cap) return false;
    arena[used++] = c;
    return true;
  }
  bool emit_cp(uint32_t cp) {
    if (cp < 0x80) return emit((char)cp);
    if (cp < 0x800) return emit((char)(0xC0 | (cp >> 6))) && emit((char)(0x80 | (cp & 0x3F)));
    if (cp < 0x10000)
      return emit((char)(0xE0 | (cp >> 12))) && emit((char)(0x80 | ((cp >> 6) & 0x3F))) &&
             emit((char)(0x80 | (cp & 0x3F)));
    return emit((char)(0xF0 | (cp >> 18))) && emit((char)(0x80 | ((cp >> 12) & 0x3F))) &&
           emit((char)(0x80 | ((cp >> 6) & 0x3F))) && emit((char)(0x80 | (cp & 0x3F)));
  }
  bool hex4(uint32_t* v) {
    if (e - p < 4) return false;
    uint32_t x = 0;
    for (int i = 0; i < 4; ++i) {
      const char c = p[i];
      x <<= 4;
      if (c >= '0' && c <= '9') x |= (uint32_t)(c - '0');
      else if (c >= 'a' && c <= 'f') x |= (uint32_t)(c - 'a' + 10);
      else if (c >= 'A' && c <= 'F') x |= (uint32_t)(c - 'A' + 10);
      else return false;
    }
    p += 4;
    *v = x;
    return true;
  }
  // The bytes of a string up to its closing quote when it has no escape or control character: 8 per step (SWAR:
  // a byte equal to '"' or '\\', or below 0x20, stops the word loop), then byte by byte; q = where it stopped.
  static inline bool special8(uint64_t w) {
    constexpr uint64_t ones = 0x0101010101010101ull, high = 0x8080808080808080ull;
    const uint64_t quote = w ^ (ones * '"'), bslash = w ^ (ones * '\\');
    return (((quote - ones) & ~quote) | ((bslash - ones) & ~bslash) | ((w - ones * 0x20) & ~w)) & high;
  }
  const char* plain_end(const char* q) const {
    while (e - q >= 8 && !special8(load8(q))) q += 8;
    while (q < e && *q != '"' && *q != '\\' && (unsigned char)*q >= 0x20) ++q;
    return q;
  }
  // A string in place (no copy) when it has no escape -- the keys, the hex digest and signature; else unescaped into
  // the arena (the caller restores `used` after reading it).
  bool view(const char** s, size_t* n) {
    ws();
    if (p >= e || *p != '"') return false;
    const char* q = plain_end(p + 1);
    if (q < e && *q == '"') {
      *s = p + 1;
      *n = (size_t)(q - p - 1);
      p = q + 1;
      return true;
    }
    return str(s, n, true);
  }
  // string -> arena (store=true) or validated and skipped; *s/*n describe the unescaped bytes
  bool str(const char** s, size_t* n, bool store) {
    ws();
    if (p >= e || *p != '"') return false;
    ++p;
    const size_t start = used;
    {  // the common case: no escape -- one copy
      const char* q = plain_end(p);
      if (q < e && *q == '"') {
        const size_t k = (size_t)(q - p);
        if (store) {
          if (!arena || cap - used < k) return false;
          memcpy(arena + used, p, k);
          used += k;
        }
        p = q + 1;
        if (s) *s = store ? arena + start : nullptr;
        if (n) *n = k;
        return true;
      }
    }
    while (true) {
      if (p >= e) return false;
      const unsigned char c = (unsigned char)*p++;
      if (c == '"') break;
      if (c < 0x20) return false;
      if (c != '\\') {
        if (store && !emit((char)c)) return false;
        continue;
      }
      if (p >= e) return false;
      const char x = *p++;
      char o;
      switch (x) {
        case '"': o = '"'; break;
        case '\\': o = '\\'; break;
        case '/': o = '/'; break;
        case 'b': o = '\b'; break;
        case 'f': o = '\f'; break;
        case 'n': o = '\n'; break;
        case 'r': o = '\r'; break;
        case 't': o = '\t'; break;
        case 'u': {
          uint32_t cp;
          if (!hex4(&cp)) return false;
          if (cp >= 0xDC00 && cp <= 0xDFFF) return false;  // lone low surrogate
          if (cp >= 0xD800 && cp <= 0xDBFF) {
            uint32_t lo;
            if (e - p < 6 || p[0] != '\\' || p[1] != 'u') return false;
            p += 2;
            if (!hex4(&lo) || lo < 0xDC00 || lo > 0xDFFF) return false;
            cp = 0x10000 + ((cp - 0xD800) << 10) + (lo - 0xDC00);
          }
          if (store && !emit_cp(cp)) return false;
          continue;
        }
        default: return false;
      }
      if (store && !emit(o)) return false;
    }
    if (s) *s = store ? arena + start : nullptr;
    if (n) *n = used - start;
    return true;
  }
  char kbuf[64];
  bool key(const char** s, size_t* n) {
    // keys are short: in place, or (escaped) unescaped into a private buffer (the caller compares immediately)
    char* a = arena;
    const size_t c = cap, u = used;
    arena = kbuf; cap = sizeof kbuf; used = 0;
    const bool ok = view(s, n);
    arena = a; cap = c; used = u;
    return ok && lit(':');
  }
  bool u64(uint64_t* v) {
    ws();
    if (p >= e || *p < '0' || *p > '9') return false;
    if (*p == '0' && p + 1 < e && p[1] >= '0' && p[1] <= '9') return false;  // leading zero
    uint64_t x = 0;
    while (p < e && *p >= '0' && *p <= '9') {
      const uint64_t d = (uint64_t)(*p - '0');
      if (x > (UINT64_MAX - d) / 10) return false;
      x = x * 10 + d;
      ++p;
    }
    if (p < e && (*p == '.' || *p == 'e' || *p == 'E')) return false;  // a float is not a u64
    *v = x;
    return true;
  }
  bool skip_value(int depth = 0) {
    if (depth > 64) return false;
    ws();
    if (p >= e) return false;
    const char c = *p;
    if (c == '"') return str(nullptr, nullptr, false);
    if (c == '{' || c == '[') {
      const char close = c == '{' ? '}' : ']';
      ++p;
      if (lit(close)) return true;
      while (true) {
        if (c == '{') {
          if (!str(nullptr, nullptr, false) || !lit(':')) return false;
        }
        if (!skip_value(depth + 1)) return false;
        if (lit(',')) continue;
        return lit(close);
      }
    }
    if (c == '-' || (c >= '0' && c <= '9')) {
      ++p;
      while (p < e && ((*p >= '0' && *p <= '9') || *p == '.' || *p == 'e' || *p == 'E' || *p == '+' || *p == '-'))
        ++p;
      return true;
    }
    static const char* const WORDS[3] = {"true", "false", "null"};
    for (const char* w : WORDS) {
      const size_t k = strlen(w);
      if ((size_t)(e - p) >= k && memcmp(p, w, k) == 0) { p += k; return true; }
    }
    return false;
  }
};

bool eq(const char* s, size_t n, const char* lit_) { return strlen(lit_) == n && memcmp(s, lit_, n) == 0; }

// lowercase hex digit values (format!("{:x}") is lowercase), 0xFF for anything else
struct HexTable {
  uint8_t v[256];
  constexpr HexTable() : v() {
    for (int c = 0; c < 256; ++c) v[c] = 0xFF;
    for (int c = '0'; c <= '9'; ++c) v[c] = (uint8_t)(c - '0');
    for (int c = 'a'; c <= 'f'; ++c) v[c] = (uint8_t)(c - 'a' + 10);
  }
};
constexpr HexTable HEX_VAL{};
// 8 lowercase hex characters -> 4 bytes, SWAR; false if any is not one of 0-9a-f.  Per character: value = low
// nibble + 9 if bit 6 is set (letters); valid iff the value is < 16 and maps back to exactly that character.
static inline bool hex8(const char* s, uint32_t* out) {
  constexpr uint64_t ones = 0x0101010101010101ull, high = 0x8080808080808080ull;
  const uint64_t w = load8(s);
  const uint64_t val = (w & (ones * 0x0F)) + ((w >> 6) & ones) * 9;
  const uint64_t gt9 = ((val + ones * 0x76) & high) >> 7;
  const uint64_t recon = val + ones * 0x30 + gt9 * 0x27;
  uint64_t x = ((val & 0x00FF00FF00FF00FFull) << 4) | ((val >> 8) & 0x00FF00FF00FF00FFull);
  x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
  x = (x | (x >> 16)) & 0xFFFFFFFFull;
  *out = (uint32_t)x;
  return recon == w && !((val + ones * 0x70) & high);
}
#if defined(__SSE2__)
// 16 lowercase hex characters -> 8 bytes (one 8-byte store), SSE2 (the x86-64 baseline); the same rule as hex8
static inline bool hex16_sse2(const char* s, uint8_t* out) {
  const __m128i c = _mm_loadu_si128((const __m128i*)s);
  const __m128i letter = _mm_cmpeq_epi8(_mm_and_si128(c, _mm_set1_epi8(0x40)), _mm_set1_epi8(0x40));
  const __m128i val = _mm_add_epi8(_mm_and_si128(c, _mm_set1_epi8(0x0F)), _mm_and_si128(letter, _mm_set1_epi8(9)));
  const __m128i gt9 = _mm_cmpgt_epi8(val, _mm_set1_epi8(9));
  const __m128i recon = _mm_add_epi8(_mm_add_epi8(val, _mm_set1_epi8(0x30)), _mm_and_si128(gt9, _mm_set1_epi8(0x27)));
  const __m128i bad = _mm_or_si128(_mm_xor_si128(_mm_cmpeq_epi8(recon, c), _mm_set1_epi8(-1)),
                                   _mm_cmpgt_epi8(val, _mm_set1_epi8(15)));
  // (byte 2k holds the high nibble of output byte k: 16-bit lanes (lo << 4) | hi, packed to bytes)
  const __m128i pairs = _mm_or_si128(_mm_slli_epi16(_mm_and_si128(val, _mm_set1_epi16(0x00FF)), 4),
                                     _mm_srli_epi16(val, 8));
  _mm_storel_epi64((__m128i*)out, _mm_packus_epi16(pairs, pairs));
  return _mm_movemask_epi8(bad) == 0;
}
#endif
bool parse_hex(const char* s, size_t n, uint8_t* out, size_t nbytes) {
  if (n != 2 * nbytes) return false;
  size_t i = 0;
  bool ok = true;
#if defined(__SSE2__)
  for (; i + 8 <= nbytes; i += 8) ok &= hex16_sse2(s + 2 * i, out + i);
#endif
  // (8 output bytes per store: the digest and signature are read back 8 bytes at a time -- push's compare and row
  // copy -- and 4-byte stores under 8-byte loads would defeat store-to-load forwarding)
  for (; i + 8 <= nbytes; i += 8) {
    uint32_t lo, hi;
    ok &= hex8(s + 2 * i, &lo);
    ok &= hex8(s + 2 * i + 8, &hi);
    const uint64_t v = (uint64_t)lo | (uint64_t)hi << 32;
    memcpy(out + i, &v, 8);
  }
  uint8_t bad = 0;
  for (; i < nbytes; ++i) {
    const uint8_t hi = HEX_VAL.v[(uint8_t)s[2 * i]], lo = HEX_VAL.v[(uint8_t)s[2 * i + 1]];
    bad |= (uint8_t)(hi | lo);
    out[i] = (uint8_t)(hi << 4 | (lo & 15));
  }
  return ok && !(bad & 0x80);  // (every valid digit is < 16: an invalid one sets the top bit)
}

bool parse_client_request(Parser& P, pbft_wire_msg* m) {
  if (!P.lit('{')) return false;
  bool has_op = false, has_ts = false, has_cl = false;
  if (!P.lit('}')) {
    do {
      const char* k;
      size_t kn;
      if (!P.key(&k, &kn)) return false;
      if (eq(k, kn, "operation")) {
        if (has_op) return false;
        const char* s;
        size_t n;
        if (!P.str(&s, &n, true)) return false;
        m->operation = s;
        m->operation_len = (uint32_t)n;
        has_op = true;
      } else if (eq(k, kn, "timestamp")) {
        if (has_ts || !P.u64(&m->timestamp)) return false;
        has_ts = true;
      } else if (eq(k, kn, "client")) {
        if (has_cl) return false;
        const size_t mark = P.used;
        const char* s;
        size_t n;
        if (!P.str(&s, &n, true) || n == 0 || n >= sizeof m->client) return false;
        memcpy(m->client, s, n);
        m->client[n] = 0;
        P.used = mark;
        has_cl = true;
      } else if (!P.skip_value()) {
        return false;
      }
    } while (P.lit(','));
    if (!P.lit('}')) return false;
  }
  return has_op && has_ts && has_cl;
}

bool parse_body(Parser& P, uint32_t kind, pbft_wire_msg* m) {
  if (kind == PBFT_MSG_CLIENT_REQUEST) return parse_client_request(P, m);
  if (!P.lit('{')) return false;
  bool has_v = false, has_n = false, has_d = false, has_m = false, has_r = false, has_s = false;
  if (!P.lit('}')) {
    do {
      const char* k;
      size_t kn;
      if (!P.key(&k, &kn)) return false;
      if (eq(k, kn, "view")) {
        if (has_v || !P.u64(&m->view)) return false;
        has_v = true;
      } else if (eq(k, kn, "sequence_number")) {
        if (has_n || !P.u64(&m->seq)) return false;
        has_n = true;
      } else if (eq(k, kn, "digest")) {
        if (has_d) return false;
        const size_t mark = P.used;
        const char* s;
        size_t n;
        if (!P.view(&s, &n)) return false;
        m->digest_ok = parse_hex(s, n, m->digest, 64) ? 1u : 0u;
        P.used = mark;
        has_d = true;
      } else if (kind == PBFT_MSG_PREPREPARE && eq(k, kn, "message")) {
        if (has_m || !parse_client_request(P, m)) return false;
        has_m = true;
      } else if (eq(k, kn, "replica")) {
        uint64_t r;
        if (has_r || !P.u64(&r) || r > 0xFFFFu) return false;
        m->replica = (uint32_t)r;
        has_r = true;
      } else if (eq(k, kn, "signature")) {
        if (has_s) return false;
        const size_t mark = P.used;
        const char* s;
        size_t n;
        if (!P.view(&s, &n) || !parse_hex(s, n, m->sig, 64)) return false;
        P.used = mark;
        has_s = true;
      } else if (!P.skip_value()) {
        return false;
      }
    } while (P.lit(','));
    if (!P.lit('}')) return false;
  }
  if (has_r != has_s) return false;  // the extension comes as a pair
  m->has_sig = has_s ? 1u : 0u;
  return has_v && has_n && has_d && (kind != PBFT_MSG_PREPREPARE || has_m);
}

// The canonical compact form of a signed vote, exactly as serde_json (and pbft_wire_encode_json) writes it:
//   {"Prepare":{"view":V,"sequence_number":N,"digest":"<128 hex>","replica":R,"signature":"<128 hex>"}}
// (or "Commit") matched byte for byte, numbers and hex decoded in place (r06: the single-message JSON ingress).
// Every byte it accepts is ASCII it checked, so no UTF-8 pass is needed; anything else -- whitespace, another field
// order, an escape, unknown fields, a PrePrepare or an unsigned vote, an invalid number or hex digit -- returns
// false and the general parser decides, with serde's rules, exactly as it did before.
bool fast_vote(const char* s, size_t n, pbft_wire_msg* m) {
  const char* p = s;
  const char* const e = s + n;
  auto lit = [&](const char* L, size_t k) {
    if ((size_t)(e - p) < k || memcmp(p, L, k) != 0) return false;
    p += k;
    return true;
  };
  auto num = [&](uint64_t* v) {  // (the general parser's u64 rules: digits, no leading zero, no overflow)
    if (p >= e || *p < '0' || *p > '9' || (*p == '0' && p + 1 < e && p[1] >= '0' && p[1] <= '9')) return false;
    uint64_t x = 0;
    for (; p < e && *p >= '0' && *p <= '9'; ++p) {
      const uint64_t d = (uint64_t)(*p - '0');
      if (x > (UINT64_MAX - d) / 10) return false;
      x = x * 10 + d;
    }
    *v = x;
    return true;
  };
  auto hex64 = [&](uint8_t* out) {
    if (e - p < 129 || p[128] != '"' || !parse_hex(p, 128, out, 64)) return false;
    p += 129;
    return true;
  };
  uint32_t kind;
  if (lit("{\"Prepare\":{\"view\":", 19)) kind = PBFT_MSG_PREPARE;
  else if (lit("{\"Commit\":{\"view\":", 18)) kind = PBFT_MSG_COMMIT;
  else return false;
  uint64_t view, seq, rep;
  if (!num(&view) || !lit(",\"sequence_number\":", 19) || !num(&seq) || !lit(",\"digest\":\"", 11) ||
      !hex64(m->digest) || !lit(",\"replica\":", 11) || !num(&rep) || rep > 0xFFFFu ||
      !lit(",\"signature\":\"", 14) || !hex64(m->sig) || !lit("}}", 2) || p != e)
    return false;
  m->kind = kind;
  m->view = view;
  m->seq = seq;
  m->digest_ok = 1;
  m->has_sig = 1;
  m->replica = (uint32_t)rep;
  return true;
}

}  // namespace

extern "C" {

size_t pbft_uvi_encode(uint64_t v, uint8_t out[10]) {
  size_t n = 0;
  do {
    uint8_t b = (uint8_t)(v & 0x7F);
    v >>= 7;
    if (v) b |= 0x80;
    out[n++] = b;
  } while (v);
  return n;
}

int pbft_uvi_decode(const uint8_t* buf, size_t len, uint64_t* value, size_t* header_bytes) {
  if (!value || !header_bytes || (!buf && len)) return PBFT_EINVAL;
  uint64_t v = 0;
  for (size_t i = 0; i < 10; ++i) {
    if (i >= len) return 1;  // need more bytes
    const uint8_t b = buf[i];
    if (i == 9 && b > 1) return PBFT_EINVAL;  // > u64
    v |= (uint64_t)(b & 0x7F) << (7 * i);
    if (!(b & 0x80)) {
      if (b == 0 && i > 0) return PBFT_EINVAL;  // non-minimal (unsigned-varint rejects it)
      *value = v;
      *header_bytes = i + 1;
      return 0;
    }
  }
  return PBFT_EINVAL;
}

int pbft_wire_encode_json(const pbft_wire_msg* m, char* out, size_t cap, size_t* len) {
  if (!m || !len || (!out && cap)) return PBFT_EINVAL;
  Out o{out, cap};
  switch (m->kind) {
    case PBFT_MSG_CLIENT_REQUEST:
      o.puts("{\"ClientRequest\":");
      write_client_request(o, m);
      o.put('}');
      break;
    case PBFT_MSG_PREPREPARE:
    case PBFT_MSG_PREPARE:
    case PBFT_MSG_COMMIT:
      o.puts(m->kind == PBFT_MSG_PREPREPARE ? "{\"PrePrepare\":" : m->kind == PBFT_MSG_PREPARE ? "{\"Prepare\":"
                                                                                                : "{\"Commit\":");
      o.puts("{\"view\":");
      o.u64(m->view);
      o.puts(",\"sequence_number\":");
      o.u64(m->seq);
      o.puts(",\"digest\":");
      o.hex(m->digest, 64);
      if (m->kind == PBFT_MSG_PREPREPARE) {
        o.puts(",\"message\":");
        write_client_request(o, m);
      }
      if (m->has_sig) {
        if (m->replica > 0xFFFFu) return PBFT_EINVAL;
        o.puts(",\"replica\":");
        o.u64(m->replica);
        o.puts(",\"signature\":");
        o.hex(m->sig, 64);
      }
      o.puts("}}");
      break;
    default:
      return PBFT_EINVAL;
  }
  *len = o.n;
  return o.n <= cap ? 0 : PBFT_EINVAL;
}

int pbft_wire_encode_frame(const pbft_wire_msg* m, uint8_t* out, size_t cap, size_t* len) {
  if (!len) return PBFT_EINVAL;
  size_t jl = 0;
  const int rc = pbft_wire_encode_json(m, nullptr, 0, &jl);  // length probe
  if (rc && jl == 0) return PBFT_EINVAL;
  if (jl > PBFT_UVI_MAX_FRAME) return PBFT_EINVAL;
  uint8_t hdr[10];
  const size_t hn = pbft_uvi_encode(jl, hdr);
  *len = hn + jl;
  if (!out || cap < hn + jl) return PBFT_EINVAL;
  memcpy(out, hdr, hn);
  return pbft_wire_encode_json(m, (char*)out + hn, jl, &jl);
}

int pbft_wire_decode_json(const char* json, size_t len, pbft_wire_msg* out, char* arena, size_t arena_cap) {
  if (!json || !out) return PBFT_EINVAL;
  memset(out, 0, sizeof *out);
  if (fast_vote(json, len, out)) return 0;
  memset(out, 0, sizeof *out);  // (a partial fast match may have written the digest)
  if (!utf8_valid((const unsigned char*)json, len)) return PBFT_EINVAL;
  Parser P{json, json + len, arena, arena_cap};
  if (!P.lit('{')) return PBFT_EINVAL;
  const char* k;
  size_t kn;
  if (!P.key(&k, &kn)) return PBFT_EINVAL;
  uint32_t kind;
  if (eq(k, kn, "PrePrepare")) kind = PBFT_MSG_PREPREPARE;
  else if (eq(k, kn, "Prepare")) kind = PBFT_MSG_PREPARE;
  else if (eq(k, kn, "Commit")) kind = PBFT_MSG_COMMIT;
  else if (eq(k, kn, "ClientRequest")) kind = PBFT_MSG_CLIENT_REQUEST;
  else return PBFT_EINVAL;
  out->kind = kind;
  if (!parse_body(P, kind, out)) return PBFT_EINVAL;
  if (!P.lit('}')) return PBFT_EINVAL;
  P.ws();
  return P.p == P.e ? 0 : PBFT_EINVAL;  // trailing characters: serde_json errors
}

int pbft_wire_decode_votes(const uint8_t* stream, size_t len, uint32_t n_replicas, uint64_t max_frames,
                           uint64_t max_rows, uint8_t* status, uint8_t* R, uint8_t* S, uint16_t* key_idx,
                           uint8_t* msg, uint8_t* kind, uint64_t* view, uint64_t* seq, uint64_t* n_frames,
                           uint64_t* n_rows, uint64_t* consumed) {
  if (!n_frames || !n_rows || !consumed || (!stream && len)) return PBFT_EINVAL;
  if (max_rows && (!R || !S || !key_idx || !msg)) return PBFT_EINVAL;
  *n_frames = *n_rows = *consumed = 0;
  size_t off = 0;
  // small arena: votes carry no operation; a PrePrepare's operation is parsed
  // (and validated) but only its status is reported here
  static thread_local char arena[1 << 16];
  while (off < len && *n_frames < max_frames && *n_rows < max_rows) {
    uint64_t fl;
    size_t hn;
    const int rc = pbft_uvi_decode(stream + off, len - off, &fl, &hn);
    if (rc == 1) break;
    if (rc != 0 || fl > PBFT_UVI_MAX_FRAME) return PBFT_EINVAL;
    if (len - off - hn < fl) break;  // incomplete frame: keep for the next call
    const char* js = (const char*)stream + off + hn;
    pbft_wire_msg m;
    uint8_t st = PBFT_WIRE_OK;
    if (pbft_wire_decode_json(js, (size_t)fl, &m, arena, sizeof arena) != 0) st = PBFT_WIRE_EJSON;
    else if (m.kind == PBFT_MSG_CLIENT_REQUEST) st = PBFT_WIRE_EKIND;  // signed PrePrepares pass: kind-0 rows
    else if (!m.digest_ok) st = PBFT_WIRE_EDIGEST;
    else if (!m.has_sig) st = PBFT_WIRE_EUNSIGNED;
    else if (m.replica >= n_replicas) st = PBFT_WIRE_ESIGNER;
    if (status) status[*n_frames] = st;
    if (st == PBFT_WIRE_OK) {
      const uint64_t r = (*n_rows)++;
      memcpy(R + 32 * r, m.sig, 32);
      memcpy(S + 32 * r, m.sig + 32, 32);
      key_idx[r] = (uint16_t)m.replica;
      pbft_envelope(msg + PBFT_ENVELOPE_BYTES * r, (uint8_t)m.kind, m.view, m.seq, m.digest);
      if (kind) kind[r] = (uint8_t)m.kind;
      if (view) view[r] = m.view;
      if (seq) seq[r] = m.seq;
    }
    ++*n_frames;
    off += hn + (size_t)fl;
    *consumed = off;
  }
  return 0;
}

int pbft_wire_frame_index(const uint8_t* stream, size_t len, uint64_t max_frames, uint64_t* off, uint32_t* flen,
                          uint64_t* n_frames, uint64_t* consumed) {
  if (!n_frames || !consumed || (!stream && len) || (max_frames && (!off || !flen))) return PBFT_EINVAL;
  *n_frames = *consumed = 0;
  size_t at = 0;
  while (at < len && *n_frames < max_frames) {  // (the framing loop of pbft_wire_decode_votes)
    uint64_t fl;
    size_t hn;
    const int rc = pbft_uvi_decode(stream + at, len - at, &fl, &hn);
    if (rc == 1) break;
    if (rc != 0 || fl > PBFT_UVI_MAX_FRAME) return PBFT_EINVAL;
    if (len - at - hn < fl) break;  // incomplete frame: keep for the next call
    off[*n_frames] = at + hn;
    flen[*n_frames] = (uint32_t)fl;
    ++*n_frames;
    at += hn + (size_t)fl;
    *consumed = at;
  }
  return 0;
}

int pbft_wire_encode_votes(uint64_t N, const uint8_t* kind, const uint64_t* view, const uint64_t* seq,
                           const uint8_t* digests, const uint32_t* replica, const uint8_t* sigs, uint8_t* out,
                           size_t cap, size_t* len) {
  if (!len || (N && (!kind || !view || !seq || !digests || !replica || !sigs))) return PBFT_EINVAL;
  size_t off = 0;
  int rc = 0;
  for (uint64_t i = 0; i < N; ++i) {
    pbft_wire_msg m;
    memset(&m, 0, sizeof m);
    m.kind = kind[i];
    m.view = view[i];
    m.seq = seq[i];
    memcpy(m.digest, digests + 64 * i, 64);
    m.digest_ok = 1;
    m.has_sig = 1;
    m.replica = replica[i];
    memcpy(m.sig, sigs + 64 * i, 64);
    if (m.kind != PBFT_MSG_PREPARE && m.kind != PBFT_MSG_COMMIT) return PBFT_EINVAL;
    size_t fl = 0;
    const bool room = out && off <= cap;
    const int e = pbft_wire_encode_frame(&m, room ? out + off : nullptr, room ? cap - off : 0, &fl);
    if (fl == 0) return PBFT_EINVAL;
    if (e) rc = PBFT_EINVAL;  // (no room: keep counting the length)
    off += fl;
  }
  *len = off;
  return rc;
}

// The primary's side of pbft_wire_encode_votes.  A canonical request's frame comes from propose_core.h's writer (the
// one the device runs), every other one from pbft_wire_encode_frame.
int pbft_wire_encode_preprepares(uint64_t N, uint64_t view, uint64_t first_seq, const uint8_t* ops,
                                 const uint64_t* op_off, const uint32_t* op_len, const uint64_t* timestamp,
                                 const char* clients, uint32_t replica, const uint8_t* digests, const uint8_t* sigs,
                                 uint8_t* out, size_t cap, size_t* len, uint64_t* frame_off, uint8_t* status) {
  if (!len) return PBFT_EINVAL;
  *len = 0;
  if ((!out && cap) || replica > pbft::PR_MAX_REPLICA) return PBFT_EINVAL;
  if (N && (!op_off || !op_len || !timestamp || !clients || first_seq + (N - 1) < first_seq)) return PBFT_EINVAL;
  const bool query = !out && cap == 0;
  if (N && !query && (!digests || !sigs)) return PBFT_EINVAL;
  static const uint8_t zero[64] = {0};
  size_t off = 0;
  int rc = 0;
  for (uint64_t i = 0; i < N; ++i) {
    const uint8_t* op = ops ? ops + op_off[i] : nullptr;
    if (!op && op_len[i]) return PBFT_EINVAL;
    const uint8_t* cl = (const uint8_t*)clients + pbft::PR_CLIENT_FIELD * i;
    const uint32_t cl_len = pbft::pr_client_len(cl);
    const uint8_t* dg = digests ? digests + 64 * i : zero;
    const uint8_t* sg = sigs ? sigs + 64 * i : zero;
    const uint64_t seq = first_seq + i;
    if (frame_off) frame_off[i] = off;
    size_t fl = 0;
    if (pbft::pr_canonical(op, op_len[i], cl, cl_len)) {
      if (status) status[i] = PBFT_PROPOSE_OK;
      fl = pbft::pr_frame_len(view, seq, timestamp[i], replica, op_len[i], cl_len);
      if (out && off <= cap && cap - off >= fl) {
        uint32_t dw[16], sw[16];
        memcpy(dw, dg, 64);
        memcpy(sw, sg, 64);
        uint8_t* dst = out + off;
        auto put = [dst](uint32_t pos, uint8_t b) { dst[pos] = b; };
        pbft::pr_write_frame(put, view, seq, dw, op, op_len[i], timestamp[i], cl, cl_len, replica, sw);
      } else {
        rc = PBFT_EINVAL;  // (no room: keep counting the length)
      }
    } else {
      if (status) status[i] = PBFT_PROPOSE_GENERAL;
      pbft_wire_msg m;
      memset(&m, 0, sizeof m);
      m.kind = PBFT_MSG_PREPREPARE;
      m.view = view;
      m.seq = seq;
      memcpy(m.digest, dg, 64);
      m.digest_ok = 1;
      m.has_sig = 1;
      m.replica = replica;
      memcpy(m.sig, sg, 64);
      m.operation = (const char*)op;
      m.operation_len = op_len[i];
      m.timestamp = timestamp[i];
      memcpy(m.client, cl, sizeof m.client);
      const bool room = out && off <= cap;
      const int e = pbft_wire_encode_frame(&m, room ? out + off : nullptr, room ? cap - off : 0, &fl);
      if (fl == 0) return PBFT_EINVAL;
      if (e) rc = PBFT_EINVAL;
    }
    off += fl;
  }
  if (frame_off) frame_off[N] = off;
  *len = off;
  return query ? 0 : rc;
}

// ---- client replies (include/pbft_wire.h; text rule: reply_core.h) ----
namespace {

// Blake2b-512 (RFC 7693, unkeyed) of two byte strings back to back, for the reply digest D = H(C | result); the
// device's form is digest_kernels.h's.
struct Blake2b {
  uint64_t h[8];
  uint8_t buf[128];
  size_t fill = 0;
  uint64_t t = 0;
  static uint64_t rotr(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }
  Blake2b() {
    static const uint64_t IV[8] = {0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL,
                                   0xa54ff53a5f1d36f1ULL, 0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL,
                                   0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
    memcpy(h, IV, sizeof h);
    h[0] ^= 0x01010040ULL;
  }
  void compress(bool last) {
    static const uint64_t IV[8] = {0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL,
                                   0xa54ff53a5f1d36f1ULL, 0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL,
                                   0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
    static const uint8_t SIG[12][16] = {
        {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
        {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
        {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
        {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
        {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0},
        {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}};
    uint64_t m[16], v[16];
    for (int i = 0; i < 16; ++i) {
      m[i] = 0;
      for (int j = 7; j >= 0; --j) m[i] = (m[i] << 8) | buf[8 * i + j];
    }
    for (int i = 0; i < 8; ++i) { v[i] = h[i]; v[8 + i] = IV[i]; }
    v[12] ^= t;
    if (last) v[14] = ~v[14];
    auto G = [&](int a, int b, int c, int d, uint64_t x, uint64_t y) {
      v[a] = v[a] + v[b] + x; v[d] = rotr(v[d] ^ v[a], 32);
      v[c] = v[c] + v[d];     v[b] = rotr(v[b] ^ v[c], 24);
      v[a] = v[a] + v[b] + y; v[d] = rotr(v[d] ^ v[a], 16);
      v[c] = v[c] + v[d];     v[b] = rotr(v[b] ^ v[c], 63);
    };
    for (int r = 0; r < 12; ++r) {
      const uint8_t* s = SIG[r];
      G(0, 4, 8, 12, m[s[0]], m[s[1]]);   G(1, 5, 9, 13, m[s[2]], m[s[3]]);
      G(2, 6, 10, 14, m[s[4]], m[s[5]]);  G(3, 7, 11, 15, m[s[6]], m[s[7]]);
      G(0, 5, 10, 15, m[s[8]], m[s[9]]);  G(1, 6, 11, 12, m[s[10]], m[s[11]]);
      G(2, 7, 8, 13, m[s[12]], m[s[13]]); G(3, 4, 9, 14, m[s[14]], m[s[15]]);
    }
    for (int i = 0; i < 8; ++i) h[i] ^= v[i] ^ v[8 + i];
  }
  void update(const uint8_t* p, size_t n) {
    while (n) {
      if (fill == 128) {  // (a full buffer is compressed only when more follows: the last block is final's)
        t += 128;
        compress(false);
        fill = 0;
      }
      const size_t k = n < 128 - fill ? n : 128 - fill;
      memcpy(buf + fill, p, k);
      fill += k;
      p += k;
      n -= k;
    }
  }
  void final(uint8_t out[64]) {
    t += fill;
    memset(buf + fill, 0, 128 - fill);
    compress(true);
    for (int i = 0; i < 8; ++i)
      for (int j = 0; j < 8; ++j) out[8 * i + j] = (uint8_t)(h[i] >> (8 * j));
  }
};

}  // namespace

int pbft_reply_digests(uint64_t N, const char* clients, const uint8_t* results, uint64_t results_bytes,
                       const uint64_t* res_off, const uint32_t* res_len, uint8_t* digests_out) {
  if (N && (!clients || !res_off || !res_len || !digests_out)) return PBFT_EINVAL;
  if (results_bytes && !results) return PBFT_EINVAL;
  for (uint64_t i = 0; i < N; ++i)
    if (res_len[i] > results_bytes || res_off[i] > results_bytes - res_len[i]) return PBFT_EINVAL;
  for (uint64_t i = 0; i < N; ++i) {
    uint8_t c[pbft::RP_CLIENT_FIELD];
    pbft::rp_client_norm(c, (const uint8_t*)clients + pbft::RP_CLIENT_FIELD * i);
    Blake2b b;
    b.update(c, sizeof c);
    if (res_len[i]) b.update(results + res_off[i], res_len[i]);
    b.final(digests_out + 64 * i);
  }
  return 0;
}

int pbft_wire_encode_replies(uint64_t N, uint64_t view, const uint64_t* timestamp, const uint8_t* results,
                             const uint64_t* res_off, const uint32_t* res_len, uint32_t replica, const char* peer_id,
                             const uint8_t* sigs, uint8_t* out, size_t cap, size_t* len, uint64_t* reply_off,
                             uint8_t* status) {
  if (!len) return PBFT_EINVAL;
  *len = 0;
  if ((!out && cap) || replica > pbft::RP_MAX_REPLICA) return PBFT_EINVAL;
  if (N && (!timestamp || !res_off || !res_len)) return PBFT_EINVAL;
  const bool query = !out && cap == 0;
  if (N && !query && (!sigs || !peer_id)) return PBFT_EINVAL;
  static const uint8_t zero[64] = {0};
  static const char no_peer[pbft::RP_PEER_ID_B58 + 1] = "1111111111111111111111111111111111111111111111111111";
  const uint8_t* pid = (const uint8_t*)(peer_id ? peer_id : no_peer);
  size_t off = 0;
  int rc = 0;
  for (uint64_t i = 0; i < N; ++i) {
    const uint8_t* res = results ? results + res_off[i] : nullptr;
    if (!res && res_len[i]) return PBFT_EINVAL;
    const uint8_t* sg = sigs ? sigs + 64 * i : zero;
    if (reply_off) reply_off[i] = off;
    size_t tl = 0;
    if (pbft::rp_canonical(res, res_len[i])) {
      if (status) status[i] = PBFT_REPLY_OK;
      tl = pbft::rp_text_len(view, timestamp[i], replica, res_len[i]);
      if (out && off <= cap && cap - off >= tl) {
        uint32_t sw[16];
        memcpy(sw, sg, 64);
        uint8_t* dst = out + off;
        auto put = [dst](uint32_t pos, uint8_t b) { dst[pos] = b; };
        pbft::rp_write_text(put, view, timestamp[i], pid, res, res_len[i], replica, sw);
      } else {
        rc = PBFT_EINVAL;  // (no room: keep counting the length)
      }
    } else {
      if (status) status[i] = PBFT_REPLY_GENERAL;
      const bool room = out && off <= cap;
      Out o{room ? (char*)out + off : nullptr, room ? cap - off : 0};
      o.puts("{\"view\":");
      o.u64(view);
      o.puts(",\"timestamp\":");
      o.u64(timestamp[i]);
      o.puts(",\"peer_id\":\"");
      for (uint32_t k = 0; k < pbft::RP_PEER_ID_B58; ++k) o.put((char)pid[k]);
      o.puts("\",\"result\":");
      o.str((const char*)res, res_len[i]);
      o.puts(",\"replica\":");
      o.u64(replica);
      o.puts(",\"signature\":");
      o.hex(sg, 64);
      o.put('}');
      tl = o.n;
      if (!room || o.n > o.cap) rc = PBFT_EINVAL;
    }
    off += tl;
  }
  if (reply_off) reply_off[N] = off;
  *len = off;
  return query ? 0 : rc;
}

int pbft_wire_decode_reply(const uint8_t* text, size_t len, pbft_reply_head* out) {
  if (!text || !out) return PBFT_EINVAL;
  memset(out, 0, sizeof *out);
  pbft::rp_head h;
  if (pbft::rp_match(text, len, h) != pbft::RP_RH_OK) return 0;
  out->view = h.view;
  out->timestamp = h.timestamp;
  out->result_off = h.result_off;
  out->result_len = h.result_len;
  out->replica = h.replica;
  out->status = PBFT_RH_OK;
  memcpy(out->peer_id, h.peer_id, sizeof out->peer_id);
  memcpy(out->sig, h.sig, 64);
  return 0;
}

// The general reader of a signed ClientReply: parse_body's rules for this struct (src/message.rs:54-103 plus the two
// signed fields).  The result goes to the arena's first bytes; the peer id must be 52 base58 characters and the signature
// 128 lowercase hex characters once their escapes, if any, are decoded.
int pbft_wire_decode_reply_json(const uint8_t* text, size_t len, pbft_reply_head* out, char* arena, size_t arena_cap) {
  if (!text || !out || (!arena && arena_cap)) return PBFT_EINVAL;
  memset(out, 0, sizeof *out);
  pbft::rp_head h;
  if (pbft::rp_match(text, len, h) == pbft::RP_RH_OK) {  // the canonical text: the matcher's fields
    if (arena_cap < h.result_len) return PBFT_EINVAL;
    pbft_wire_decode_reply(text, len, out);
    if (h.result_len) memcpy(arena, text + h.result_off, h.result_len);
    return (int)h.result_len;
  }
  if (len > (size_t)0x7fffffff || !utf8_valid(text, len)) return PBFT_EINVAL;
  const char* const s0 = (const char*)text;
  Parser P{s0, s0 + len, arena, arena_cap};
  if (!P.lit('{')) return PBFT_EINVAL;
  bool has_v = false, has_t = false, has_p = false, has_res = false, has_r = false, has_s = false;
  pbft_reply_head r;
  memset(&r, 0, sizeof r);
  size_t res_n = 0;
  // a short string in place or, escaped, unescaped into a buffer of its own (the arena holds the result and nothing else)
  char sbuf[160];
  auto private_str = [&](const char** s, size_t* n) {
    char* const a = P.arena;
    const size_t c = P.cap, u = P.used;
    P.arena = sbuf; P.cap = sizeof sbuf; P.used = 0;
    const bool ok = P.view(s, n);
    P.arena = a; P.cap = c; P.used = u;
    return ok;
  };
  if (!P.lit('}')) {
    do {
      const char* k;
      const char* s;
      size_t kn, n;
      if (!P.key(&k, &kn)) return PBFT_EINVAL;
      if (eq(k, kn, "view")) {
        if (has_v || !P.u64(&r.view)) return PBFT_EINVAL;
        has_v = true;
      } else if (eq(k, kn, "timestamp")) {
        if (has_t || !P.u64(&r.timestamp)) return PBFT_EINVAL;
        has_t = true;
      } else if (eq(k, kn, "peer_id")) {
        if (has_p || !private_str(&s, &n) || n != pbft::RP_PEER_ID_B58) return PBFT_EINVAL;
        for (uint32_t i = 0; i < pbft::RP_PEER_ID_B58; ++i) {
          if (!pbft::rp_b58_char((uint8_t)s[i])) return PBFT_EINVAL;
          r.peer_id[i] = s[i];
        }
        has_p = true;
      } else if (eq(k, kn, "result")) {
        if (has_res) return PBFT_EINVAL;
        P.ws();
        const char* const open = P.p;
        P.used = 0;
        if (!P.str(&s, &res_n, true)) return PBFT_EINVAL;
        r.result_off = (uint32_t)(open + 1 - s0);
        r.result_len = (uint32_t)(P.p - 1 - (open + 1));
        has_res = true;
      } else if (eq(k, kn, "replica")) {
        uint64_t v;
        if (has_r || !P.u64(&v) || v > 0xFFFFu) return PBFT_EINVAL;
        r.replica = (uint32_t)v;
        has_r = true;
      } else if (eq(k, kn, "signature")) {
        if (has_s || !private_str(&s, &n) || !parse_hex(s, n, r.sig, 64)) return PBFT_EINVAL;
        has_s = true;
      } else if (!P.skip_value()) {
        return PBFT_EINVAL;
      }
    } while (P.lit(','));
    if (!P.lit('}')) return PBFT_EINVAL;
  }
  P.ws();
  if (P.p != P.e) return PBFT_EINVAL;  // trailing characters: serde_json errors
  if (!(has_v && has_t && has_p && has_res && has_r && has_s)) return PBFT_EINVAL;
  r.status = PBFT_RH_GENERAL;
  *out = r;
  return (int)res_n;
}

int pbft_records_pack(const uint8_t* R, const uint8_t* S, const uint16_t* key_idx, const uint8_t* msg,
                      uint32_t msg_stride, uint64_t N, uint8_t* records) {
  if (N && (!R || !S || !key_idx || !msg || !records || msg_stride < PBFT_ENVELOPE_BYTES)) return PBFT_EINVAL;
  for (uint64_t i = 0; i < N; ++i) {
    uint8_t* o = records + PBFT_RECORD_BYTES * i;
    memset(o, 0, PBFT_RECORD_BYTES);
    memcpy(o, R + 32 * i, 32);
    memcpy(o + 32, S + 32 * i, 32);
    memcpy(o + 64, msg + (size_t)msg_stride * i, PBFT_ENVELOPE_BYTES);
    o[150] = (uint8_t)(key_idx[i] & 0xFF);
    o[151] = (uint8_t)(key_idx[i] >> 8);
  }
  return 0;
}

}  // extern "C"
