"""Interval analysis for the radix-2^25.5 field code in pbft_amd/csrc/fe25519.h.

Checks that no 64-bit column accumulator of fe_mul/fe_sq can overflow and that
every u32 limb stays below 2^32, for the exact add/sub/mul sequence used by the
mixed addition (comb step) and doubling.  Run: python tools/limb_bounds.py

Importable: the bound vectors (CARRIED, P2), the interval operations (add, sub, mulmax) and the operand bounds of
every product of the comb step (MADD_PRODUCTS) and of the doubling (DBL_PRODUCTS).  tests/arith_cases.py takes every
operand bound from here and runs the code with its limbs at them.
"""
import math
E26, E25 = 1 << 26, 1 << 25
CARRIED = [E26 if i % 2 == 0 else E25 for i in range(10)]
CARRIED[1] += 1 << 14; CARRIED[5] += 1 << 14   # carry-chain overshoot allowance
CARRIED[0] = E26
P2 = [0x7FFFFDA] + [0x3FFFFFE if i % 2 else 0x7FFFFFE for i in range(1, 10)]
P4 = [2 * x for x in P2]

def add(a, b): return [x + y for x, y in zip(a, b)]
def sub(a, b, off):
    for x, o in zip(b, off): assert x <= o, "sub underflow"
    return [x + o for x, o in zip(a, off)]
def mulmax(f, g):
    worst, cols = 0, []
    for k in range(10):
        s = 0
        for i in range(10):
            for j in range(10):
                if (i + j) % 10 != k: continue
                c = 2 if (i % 2 and j % 2) else 1
                if i + j >= 10: c *= 19
                s += c * f[i] * g[j]
        worst = max(worst, s)
        cols.append(s)
    for x in f + g: assert x < 2**32
    for i, x in enumerate(g): assert 19 * x < 2**32, "19*g overflows u32"
    for i, x in enumerate(f):
        if i % 2: assert 2 * x < 2**32
    if f is g:  # fe_sq precomputes 38*f_odd and 19*f_even
        for i, x in enumerate(f): assert (38 if i % 2 else 19) * x < 2**32, "fe_sq premult overflow"
    assert worst < 2**64, math.log2(worst)
    chain1(cols)
    return math.log2(worst)


def chain1(cols):
    """fe_reduce_wide with PBFT_REDUCE_1CHAIN (0 -> 1 -> ... -> 9 -> 0 x19 -> 1) on columns <= cols: the
    result must stay within CARRIED (h1 is the only limb above its width) and no step may overflow u64."""
    h = list(cols)
    for i in range(10):
        w = 26 if i % 2 == 0 else 25
        c = h[i] >> w
        h[i] = (1 << w) - 1
        if i < 9:
            h[i + 1] += c
        else:
            h[0] += 19 * c
        assert max(h) < 2**64
    c = h[0] >> 26
    h[0] = (1 << 26) - 1
    h[1] += c
    for x, b in zip(h, CARRIED):
        assert x <= b, "chain1 overshoot"

C = CARRIED
TABLE = [E26 - 1 if i % 2 == 0 else E25 - 1 for i in range(10)]   # canonical limbs (comb table entries)
# madd v2 (PBFT_MADD_V2, verify_core.h ge_madd_ab), the comb step on P = (X, Y, Z, T) carried and a canonical entry
# (qa, qb, k): a = (Y-X) qa, b = (Y+X) qb, c = T k' with k' = +-k (2p - k limb-wise for a negative digit);
# E = b - a, F = Z - c, G = Z + c, H = b + a; X3 = F*E, T3 = H*E, Y3 = H*G, Z3 = F*G
YMX = sub(C, C, P2); YPX = add(C, C)
KK = {False: C, True: P2}        # 2p - k <= 2p limb-wise (k canonical)
MADD_E = sub(C, C, P2); MADD_F = sub(C, C, P2); MADD_G = add(C, C); MADD_H = add(C, C)


def MADD_PRODUCTS(neg):
    """(first operand bound, second operand bound) of the seven products of one comb step; the second operand is
    the one premultiplied by 19."""
    return {"a": (YMX, C), "b": (YPX, C), "c": (C, KK[bool(neg)]), "X3": (MADD_F, MADD_E), "T3": (MADD_H, MADD_E),
            "Y3": (MADD_H, MADD_G), "Z3": (MADD_F, MADD_G)}


# doubling (ge25519.h ge_dbl; dbl-2008-hwcd, a = -1) of carried (X, Y, Z): three squares of carried values, the
# square of X + Y, and four products of carried E, F, G, H
DBL_XY = add(C, C)
DBL_PRODUCTS = {"A": (C, C), "B": (C, C), "C2": (C, C), "XY2": (DBL_XY, DBL_XY),
                "X": (C, C), "Y": (C, C), "T": (C, C), "Z": (C, C)}


# anykey (anykey_core.h): [k](-A) by 4-bit windows on a key seen for the first time.  Every value that crosses a step
# boundary is an fe_mul output or an fe_carry output, i.e. within CARRIED, so the three sequences close on themselves:
#  * doubling chain -> addition -> doubling: ak_dbl takes carried (X, Y, Z) and returns products (DBL_PRODUCTS; its
#    E', F', G', H' go through fe_carry, whose inputs AK_DBL_CARRY_IN stay below 2^31); ak_add_signed takes the carried
#    (X, Y, Z, T) of a doubling, of an addition or of the identity and returns products; so does the base-point
#    ge_madd_signed behind the last addition (MADD_PRODUCTS, as in the comb).
#  * the projective-Niels addition: D = Z1 * 2Z2 (carried operands) stands where the comb step has Z1, then ge_madd_ab
#    unchanged: qa, qb are the entry's carried Y2 -+ X2 (the comb's are canonical: the same bound but for the
#    carry-chain allowance), k' = +-2dT2 of a carried 2dT2 is <= 2p limb-wise like the comb's.
#  * the entry conversion ak_to_pniels: Y + X, Y - X and 2Z through fe_carry (AK_ENTRY_CARRY_IN), 2dT2 = T * 2d with
#    the canonical constant.
AK_DBL_CARRY_IN = {"H'": add(C, C), "E'": sub(C, C, P2), "G'": sub(C, C, P2), "C2": add(C, C), "F'": add(C, C)}
AK_ENTRY_CARRY_IN = {"Y+X": add(C, C), "Y-X": sub(C, C, P2), "2Z": add(C, C)}


def AK_ADD_PRODUCTS(neg):
    """Operand bounds of the eight products of ak_add_signed: D, then ge_madd_ab's seven on (X, Y, D, T)."""
    return {"D": (C, C), **MADD_PRODUCTS(neg)}


AK_ENTRY_PRODUCT = (C, TABLE)  # T * 2d


def main():
    for nm, v in {**AK_DBL_CARRY_IN, **AK_ENTRY_CARRY_IN}.items():
        assert max(v) < 2**31, nm  # fe_carry's precondition
    for neg in (False, True):
        for nm, (x, y) in AK_ADD_PRODUCTS(neg).items():  # (mulmax asserts each operand's role: 2x odd limbs, 19x)
            print("anykey add neg=%d %-3s log2 max col:" % (neg, nm), mulmax(x, y))
    print("anykey entry 2dT    log2 max col:", mulmax(*AK_ENTRY_PRODUCT))
    # mixed add (comb step): P3 + halved affine Niels ((y+x)/2, (y-x)/2, dxy) with canonical table limbs
    print("madd a=(Y-X)*ymx   log2 max col:", mulmax(YMX, C))
    print("madd b=(Y+X)*ypx   log2 max col:", mulmax(YPX, C))
    # r02 form (PBFT_MADD_V2 = 0): D = Z1 (halved table entries, no doubling of Z1); the second operand is the one
    # premultiplied by 19
    e, f, g, h = MADD_E, MADD_F, MADD_G, MADD_H
    for neg in (False, True):
        F, G = (g, f) if neg else (f, g)   # negative digit swaps d-c and d+c
        for nm, (x, y) in {"X3=F*E": (F, e), "Y3=G*H": (G, h), "Z3=dmc*dpc": (f, g), "T3=E*H": (e, h)}.items():
            print("madd neg=%d" % neg, nm, " log2 max col:", mulmax(x, y))
    # madd v2: F = D - c, G = D + c never swap
    for neg in (False, True):
        print("madd v2 neg=%d c=T*k'" % neg, " log2 max col:", mulmax(*MADD_PRODUCTS(neg)["c"]))
    for nm, key in {"X3=F*E": "X3", "T3=H*E": "T3", "Y3=H*G": "Y3", "Z3=F*G": "Z3"}.items():
        print("madd v2", nm, " log2 max col:", mulmax(*MADD_PRODUCTS(False)[key]))
    # doubling (dbl-2008-hwcd, a=-1): A=X^2, B=Y^2, C2=2Z^2, H=A+B, E=H-(X+Y)^2, G=A-B, F=C2+G
    print("dbl (X+Y)^2         log2 max col:", mulmax(*DBL_PRODUCTS["XY2"]))
    print("sq of carried       log2 max col:", mulmax(*DBL_PRODUCTS["A"]))
    # precomputation-only doubling: E, F, G, H are carried before the products
    for nm, key in {"X=E*F": "X", "Y=G*H": "Y", "T=E*H": "T", "Z=F*G": "Z"}.items():
        print("dbl", nm, " log2 max col:", mulmax(*DBL_PRODUCTS[key]))
    print("all bounds OK")


if __name__ == "__main__":
    main()
