// Test hook core: one arithmetic op of fe25519.h / sc25519.h / ge25519.h / verify_core.h on one item of raw words.
//
// debug_arith_item(op, in, out) runs the product's own function for `op` -- nothing is re-implemented here -- on
// the item's input words and stores its output words.  Field elements travel as their 10 RAW limbs (no
// fe_from_words on the way in, no fe_to_words on the way out, except in the two ops that test exactly those), so a
// test can put every limb of every operand at and around its documented bound, which no honest signature ever does.
// The same function is compiled twice: for gfx950 by debug_arith.hip (pbft_debug_arith: the device-only forms --
// mad_column10's asm block, dbl32, lane_mask, the bit-selects) and for the host by tests/native/arith_harness.cpp
// (hh_arith).  tests/arith_cases.py holds the cases and the Python-integer model; tests/test_arith.py and
// tests/test_gpu_arith.py compare.
//
// It reads `in` only, at compile-time offsets, and has no data-dependent addressing or branching: no input can
// make it fault.  Not part of the verify path.
#pragma once
#include "verify_core.h"

namespace pbft {

// Item layouts (words).  fe = 10 raw limbs; "sign" = one word, bit 0.
enum debug_arith_op : int {
  DA_FE_MUL = 0,       // f, g                       -> h
  DA_FE_SQ,            // f                          -> h
  DA_FE_MUL_PAR,       // f, g                       -> h   fe_mulT<true> (fe_reduce_par)
  DA_FE_SQ_PAR,        // f                          -> h   fe_sqT<true>
  DA_FE_MUL_CHAIN1,    // (f, g) x N                 -> h x N   fe_mul_chain<N>: N different operand pairs
  DA_FE_MUL_CHAIN3,
  DA_FE_MUL_CHAIN4,
  DA_FE_ADD,           // f, g                       -> h
  DA_FE_SUB,           // f, g                       -> h
  DA_FE_NEG,           // f                          -> h
  DA_FE_CARRY,         // f                          -> f carried
  DA_FE_TO_WORDS,      // f                          -> 8 words
  DA_FE_FROM_WORDS,    // 8 words                    -> f
  DA_FE_IS_ZERO,       // f                          -> 0 / 1
  DA_FE_IS_NEGATIVE,   // f                          -> 0 / 1
  DA_FE_EQ,            // a, b                       -> 0 / 1
  DA_GE_MADD,          // X, Y, Z, T, qa, qb, k, sign -> X3, Y3, Z3, T3   ge_madd_ab<true, false>
  DA_GE_MADD_CHAIN,    //                                                 ge_madd_ab<true, true>
  DA_GE_MADD_CHAIN_NOT,  //                          -> X3, Y3, Z3        ge_madd_ab<false, true>
  DA_GE_FROM_AB,       // qa, qb, k, sign            -> X, Y, Z, T
  DA_GE_DBL,           // X, Y, Z                    -> X3, Y3, Z3, T3
  DA_SC_REDUCE512,     // 16 words                   -> 8 words
  DA_SC_MULADD,        // a, b, c (8 words each)     -> 8 words
  DA_SC_LT_L,          // 8 words                    -> 0 / 1
  DA_NOPS
};

struct debug_arith_desc { const char* name; uint32_t win, wout; };

// name and widths of op, or nullptr (host side: the launcher and the tests' view of the layouts)
inline const debug_arith_desc* debug_arith_lookup(int op) {
  static const debug_arith_desc T[DA_NOPS] = {
      {"fe_mul", 20, 10},          {"fe_sq", 10, 10},           {"fe_mul_par", 20, 10},
      {"fe_sq_par", 10, 10},       {"fe_mul_chain1", 20, 10},   {"fe_mul_chain3", 60, 30},
      {"fe_mul_chain4", 80, 40},   {"fe_add", 20, 10},          {"fe_sub", 20, 10},
      {"fe_neg", 10, 10},          {"fe_carry", 10, 10},        {"fe_to_words", 10, 8},
      {"fe_from_words", 8, 10},    {"fe_is_zero", 10, 1},       {"fe_is_negative", 10, 1},
      {"fe_eq", 20, 1},            {"ge_madd", 71, 40},         {"ge_madd_chain", 71, 40},
      {"ge_madd_chain_not", 71, 30}, {"ge_from_ab", 31, 40},    {"ge_dbl", 30, 40},
      {"sc_reduce512", 16, 8},     {"sc_muladd", 24, 8},        {"sc_lt_L", 8, 1},
  };
  return op >= 0 && op < DA_NOPS ? &T[op] : nullptr;
}

FE_FN void da_ld(fe& h, const uint32_t* p) {
#pragma unroll
  for (int i = 0; i < 10; ++i) h.v[i] = p[i];
}
FE_FN void da_st(uint32_t* p, const fe& h) {
#pragma unroll
  for (int i = 0; i < 10; ++i) p[i] = h.v[i];
}

template <int N>
FE_FN void da_mul_chain(const uint32_t* in, uint32_t* out) {
  fe f[N], g[N], h[N];
  fe* ho[N];
  const fe* fo[N];
  const fe* go[N];
#pragma unroll
  for (int m = 0; m < N; ++m) {
    da_ld(f[m], in + 20 * m);
    da_ld(g[m], in + 20 * m + 10);
    ho[m] = &h[m]; fo[m] = &f[m]; go[m] = &g[m];
  }
  fe_mul_chain<N>(ho, fo, go);
#pragma unroll
  for (int m = 0; m < N; ++m) da_st(out + 10 * m, h[m]);
}

// the comb step as the comb calls it: in place on P
template <bool WITH_T, bool CHAIN>
FE_FN void da_madd(const uint32_t* in, uint32_t* out) {
  ge P;
  fe qa, qb, k;
  da_ld(P.X, in); da_ld(P.Y, in + 10); da_ld(P.Z, in + 20); da_ld(P.T, in + 30);
  da_ld(qa, in + 40); da_ld(qb, in + 50); da_ld(k, in + 60);
  ge_madd_ab<WITH_T, CHAIN>(P, P, qa, qb, k, (in[70] & 1u) != 0u);
  da_st(out, P.X); da_st(out + 10, P.Y); da_st(out + 20, P.Z);
  if constexpr (WITH_T) da_st(out + 30, P.T);
}

FE_FN void debug_arith_item(int op, const uint32_t* in, uint32_t* out) {
  switch (op) {
    case DA_FE_MUL: { fe f, g, h; da_ld(f, in); da_ld(g, in + 10); fe_mul(h, f, g); da_st(out, h); break; }
    case DA_FE_SQ: { fe f, h; da_ld(f, in); fe_sq(h, f); da_st(out, h); break; }
    case DA_FE_MUL_PAR: { fe f, g, h; da_ld(f, in); da_ld(g, in + 10); fe_mulT<true>(h, f, g); da_st(out, h); break; }
    case DA_FE_SQ_PAR: { fe f, h; da_ld(f, in); fe_sqT<true>(h, f); da_st(out, h); break; }
    case DA_FE_MUL_CHAIN1: da_mul_chain<1>(in, out); break;
    case DA_FE_MUL_CHAIN3: da_mul_chain<3>(in, out); break;
    case DA_FE_MUL_CHAIN4: da_mul_chain<4>(in, out); break;
    case DA_FE_ADD: { fe f, g, h; da_ld(f, in); da_ld(g, in + 10); fe_add(h, f, g); da_st(out, h); break; }
    case DA_FE_SUB: { fe f, g, h; da_ld(f, in); da_ld(g, in + 10); fe_sub(h, f, g); da_st(out, h); break; }
    case DA_FE_NEG: { fe f, h; da_ld(f, in); fe_neg(h, f); da_st(out, h); break; }
    case DA_FE_CARRY: { fe f; da_ld(f, in); fe_carry(f); da_st(out, f); break; }
    case DA_FE_TO_WORDS: {
      fe f; uint32_t w[8];
      da_ld(f, in); fe_to_words(w, f);
#pragma unroll
      for (int i = 0; i < 8; ++i) out[i] = w[i];
      break;
    }
    case DA_FE_FROM_WORDS: {
      fe h; uint32_t w[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) w[i] = in[i];
      fe_from_words(h, w); da_st(out, h);
      break;
    }
    case DA_FE_IS_ZERO: { fe f; da_ld(f, in); out[0] = fe_is_zero(f) ? 1u : 0u; break; }
    case DA_FE_IS_NEGATIVE: { fe f; da_ld(f, in); out[0] = fe_is_negative(f) ? 1u : 0u; break; }
    case DA_FE_EQ: { fe a, b; da_ld(a, in); da_ld(b, in + 10); out[0] = fe_eq(a, b) ? 1u : 0u; break; }
    case DA_GE_MADD: da_madd<true, false>(in, out); break;
    case DA_GE_MADD_CHAIN: da_madd<true, true>(in, out); break;
    case DA_GE_MADD_CHAIN_NOT: da_madd<false, true>(in, out); break;
    case DA_GE_FROM_AB: {
      ge P; fe qa, qb, k;
      da_ld(qa, in); da_ld(qb, in + 10); da_ld(k, in + 20);
      ge_from_ab(P, qa, qb, k, (in[30] & 1u) != 0u);
      da_st(out, P.X); da_st(out + 10, P.Y); da_st(out + 20, P.Z); da_st(out + 30, P.T);
      break;
    }
    case DA_GE_DBL: {  // in place, as comb_entry calls it (ge_dbl does not read T)
      ge P;
      da_ld(P.X, in); da_ld(P.Y, in + 10); da_ld(P.Z, in + 20); fe_zero(P.T);
      ge_dbl(P, P);
      da_st(out, P.X); da_st(out + 10, P.Y); da_st(out + 20, P.Z); da_st(out + 30, P.T);
      break;
    }
    case DA_SC_REDUCE512: {
      uint32_t x[16], o[8];
#pragma unroll
      for (int i = 0; i < 16; ++i) x[i] = in[i];
      sc_reduce512(o, x);
#pragma unroll
      for (int i = 0; i < 8; ++i) out[i] = o[i];
      break;
    }
    case DA_SC_MULADD: {
      uint32_t a[8], b[8], c[8], o[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) { a[i] = in[i]; b[i] = in[8 + i]; c[i] = in[16 + i]; }
      sc_muladd(o, a, b, c);
#pragma unroll
      for (int i = 0; i < 8; ++i) out[i] = o[i];
      break;
    }
    case DA_SC_LT_L: {
      uint32_t s[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) s[i] = in[i];
      out[0] = sc_lt_L(s) ? 1u : 0u;
      break;
    }
    default: break;
  }
}

}  // namespace pbft
