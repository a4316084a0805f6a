// Per-lane Ed25519 verify_strict under a key the lane sees for the first time: no installed key set, no table in HBM.
// Same semantics as verify_core.h (include/pbft_verify.h, dalek 1.0.1 verify_strict); the public key comes as 32 raw
// bytes with the signature.  Host and device (FE_FN), one signature per lane, uniform control flow.
//
//   R' = [s]B + [k](-A)
//    * A is decompressed in the lane; key_ok = it decompresses and is not of small order.
//    * [k](-A): fixed signed 4-bit windows.  k < L < 2^253 is recoded into 64 digits in [-8, 8) (the top one in
//      [0, 2]); a per-lane table holds j * (-A), j = 0 .. 8, as projective Niels entries (Y + X, Y - X, 2Z, 2dT; entry 0
//      is the identity, so a zero digit takes no branch).  From the top window down: four doublings, then one addition
//      of +-entry: 252 doublings and 64 additions.  T is computed only by the doubling in front of an addition.
//      The sign swaps the entry's first two coordinates and negates its last by masks (fe_cswap_mask,
//      fe_cneg_canon), and the addition is verify_core.h's ge_madd_ab with D = Z1 * 2Z2 in the place of Z1.
//    * [s]B: the context's base-point comb table (plan PLB), added as PLB::P mixed additions into the same
//      accumulator after the last doubling (ge_madd_signed): no separate point addition.  A rejected s (>= L) is
//      recoded as 0 (sc_clamp_rejected): no gather past the table.
//    * The table index of either part is in range for ANY input words (window digits: |d| <= 8 by construction), so a
//      test hook that passes k >= 2^253 computes a wrong point and reads nothing out of bounds.
//   Output: X, Y, Z of R' and flag = s_ok && key_ok -- the comb kernels' hand-off to finish_kernel, which inverts,
//   compares with R and tests for small order.
//
// Limb bounds of the sequences used here (doubling chain -> addition -> doubling, the projective-Niels addition,
// the entry conversion): tools/limb_bounds.py, "anykey".
#pragma once
#include "verify_core.h"

namespace pbft {

// j * (-A) as (Y + X, Y - X, 2Z, 2dT), every coordinate carried
struct pniels { fe ypx, ymx, z2, t2d; };
static constexpr int AK_WINDOWS = 64;  // 4-bit windows over 256 bits
static constexpr int AK_ENTRIES = 9;   // 0 .. 8 times -A

// r = 2p with ge_dbl's arithmetic (ge25519.h); T3 only where an addition follows.  p.X, p.Y, p.Z carried.
template <bool WITH_T>
FE_FN void ak_dbl(ge& r, const ge& p) {
  fe a, b, c, e, f, g, h, t;
  fe_sq(a, p.X);
  fe_sq(b, p.Y);
  fe_sq(c, p.Z); fe_add(c, c, c);
  fe_add(t, p.X, p.Y); fe_sq(t, t);
  fe_add(h, a, b); fe_carry(h);   // H' = A + B          (= -H)
  fe_sub(e, h, t); fe_carry(e);   // E' = H' - (X+Y)^2   (= -E)
  fe_sub(g, a, b); fe_carry(g);   // G' = A - B          (= -G)
  fe_carry(c);
  fe_add(f, c, g); fe_carry(f);   // F' = 2Z^2 + G'      (= -F)
  fe_mul(r.X, e, f); fe_mul(r.Y, g, h); fe_mul(r.Z, f, g);
  if constexpr (WITH_T) fe_mul(r.T, e, h);
}

// Projective Niels form of an extended point with carried coordinates (one multiplication)
FE_FN void ak_to_pniels(pniels& n, const ge& p) {
  fe d2;
  fe_const_2d(d2);
  fe_add(n.ypx, p.Y, p.X); fe_carry(n.ypx);
  fe_sub(n.ymx, p.Y, p.X); fe_carry(n.ymx);
  fe_add(n.z2, p.Z, p.Z); fe_carry(n.z2);
  fe_mul(n.t2d, p.T, d2);
}

// r = p + sign * q (8 multiplications; unified and complete, so p = +-q and torsion points need no special case):
//   A = (Y1 - X1) qa, B = (Y1 + X1) qb, C = T1 (+-2d T2), D = Z1 (2 Z2), then ge_madd_ab's E, F, G, H and products
// with (qa, qb) = (Y2 - X2, Y2 + X2), swapped for -q.  p's coordinates carried.
template <bool WITH_T = true>
FE_FN void ak_add_signed(ge& r, const ge& p, const pniels& q, bool neg) {
  fe qa = q.ymx, qb = q.ypx;
  fe_cswap_mask(qa, qb, lane_mask(neg));
  ge pd;
  pd.X = p.X; pd.Y = p.Y; pd.T = p.T;
  fe_mul(pd.Z, p.Z, q.z2);
  ge_madd_ab<WITH_T>(r, pd, qa, qb, q.t2d, neg);
}

// k < 2^253 as 64 signed 4-bit digits, packed as two's-complement nibbles: adding 8 to every nibble carries out of
// exactly those whose digit (nibble + carry in) is 8 or more, and leaves digit + 8 mod 16 behind; the XOR takes the 8
// off again.  The top nibble plus its carry is at most 2: no carry out of the 256 bits.
FE_FN void ak_recode(uint32_t rec[8], const uint32_t k[8]) {
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t t = (uint64_t)k[i] + 0x88888888u + c;
    rec[i] = (uint32_t)t ^ 0x88888888u;
    c = (uint32_t)(t >> 32);
  }
}

// digit of the top window, then the windows move up by one: magnitude (0 .. 8 for any input) and sign
FE_FN void ak_next_digit(uint32_t rec[8], uint32_t& mag, bool& neg) {
  const uint32_t nib = rec[7] >> 28;
  neg = nib >= 8u;
  mag = neg ? 16u - nib : nib;
#pragma unroll
  for (int i = 7; i > 0; --i) rec[i] = (rec[i] << 4) | (rec[i - 1] >> 28);
  rec[0] <<= 4;
}

// The digits of `digits` (verify_core.h) with the window width at run time, for a loop over a plan's positions
FE_FN int ak_take(digits& d, int W) {
  const int v = (int)((d.w[0] & ((1u << W) - 1u)) + d.carry);
#pragma unroll
  for (int i = 0; i < 7; ++i) d.w[i] = (d.w[i] >> W) | (d.w[i + 1] << (32 - W));
  d.w[7] >>= W;
  d.carry = (v >= (1 << (W - 1))) ? 1u : 0u;
  return v - (int)(d.carry << W);
}
FE_FN int ak_take_last(const digits& d, int W) { return (int)((d.w[0] & ((1u << W) - 1u)) + d.carry); }

// P = [s]B + [k](-A) for the key encoded by a_enc; k < 2^253.  Returns s_ok && key_ok; key_ok also on its own.
// tab: the lane's own AK_ENTRIES entries (a private array: scratch on the device, which is swizzled per lane and so
// serves a lane-varying index).
template <class PLB>
FE_FN bool anykey_sum(ge& P, const uint32_t s_in[8], const uint32_t k[8], const uint32_t a_enc[8],
                      const uint32_t* tabB, bool& key_ok) {
  pniels tab[AK_ENTRIES];
  {
    ge A;
    const bool dec = ge_decompress(A, a_enc);
    key_ok = dec && !ge_is_small_order(A);
    ge M;
    ge_neg(M, A);  // (-x, y, 1, -xy), carried
    // entry 0: the identity (1, 1, 2, 0)
    fe_one(tab[0].ypx); fe_one(tab[0].ymx); fe_zero(tab[0].z2); tab[0].z2.v[0] = 2; fe_zero(tab[0].t2d);
    ak_to_pniels(tab[1], M);
#pragma unroll 1
    for (int j = 2; j < AK_ENTRIES; ++j) {
      ak_add_signed(M, M, tab[1], false);  // j * (-A) = (j - 1) * (-A) + (-A)
      ak_to_pniels(tab[j], M);
    }
  }

  uint32_t rec[8];
  ak_recode(rec, k);
  ge_identity(P);
  // (real loops: one copy of each doubling form and of the addition in the instruction stream)
#pragma unroll 1
  for (int w = AK_WINDOWS - 1; w >= 0; --w) {
    if (w != AK_WINDOWS - 1) {
#pragma unroll 1
      for (int t = 0; t < 3; ++t) ak_dbl<false>(P, P);
      ak_dbl<true>(P, P);
    }
    uint32_t mag;
    bool neg;
    ak_next_digit(rec, mag, neg);
    ak_add_signed(P, P, tab[mag], neg);
  }

  uint32_t s[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) s[i] = s_in[i];
  const bool s_ok = sc_lt_L(s);
  sc_clamp_rejected(s, s_ok);
  digits ds;
  ds.init(s);
#pragma unroll 1
  for (int pos = 0; pos < PLB::P; ++pos) {
    const int W = PLB::width(pos);
    const int d = pos == PLB::P - 1 ? ak_take_last(ds, W) : ak_take(ds, W);
    const int ad = d < 0 ? -d : d;
    niels q;
    load_niels(q, tabB + ((size_t)PLB::offset(pos) + (uint32_t)ad) * 32);
    ge_madd_signed(P, P, q, d < 0);
  }
  return s_ok && key_ok;
}

// The whole lane up to the hand-off: the challenge hash over the raw bytes, its reduction, the sum.
template <class PLB, int LEN>
FE_FN bool anykey_lane(ge& P, const uint32_t r_enc[8], const uint32_t s[8], const uint32_t a_enc[8],
                       const uint8_t* msg, int len, const uint32_t* tabB) {
  uint32_t h[16], k[8];
  if constexpr (LEN == 85) sha512_ram85(h, r_enc, a_enc, msg, nullptr);
  else sha512_ram<LEN>(h, r_enc, a_enc, msg, len);
  sc_reduce512(k, h);
  bool key_ok;
  return anykey_sum<PLB>(P, s, k, a_enc, tabB, key_ok);
}

}  // namespace pbft
