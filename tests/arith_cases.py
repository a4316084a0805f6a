"""Cases, Python-integer model and shared checks of the arithmetic op table (pbft_amd/csrc/debug_arith_core.h):
every op of fe25519.h, sc25519.h and the comb step / doubling on RAW limbs, with every operand at and around the
bound its role is documented to have.  Used by tests/test_arith.py (host build, hh_arith) and
tests/test_gpu_arith.py (gfx950 build, pbft_debug_arith); both pass a backend with

    backend.ops                  {name: (op id, words in, words out)}, read from the hook itself
    backend.call(op, in, out, n) the hook's return code (in, out: numpy uint32 arrays or None)

Bounds come from tools/limb_bounds.py (the interval analysis of the same code) and, for fe_reduce_par, from the
figures in fe25519.h.  The value of a limb vector is sum(limb[i] << OFF[i]); every expected result is that value
pushed through the op's formula in Python integers.  The generator asserts that every vector it emits lies within
its role's bound, and nothing is filtered afterwards: every generated case is run and checked.  A value that a role
cannot represent at all (2^255 in canonical limbs) is not part of that role's list in the first place.
"""
import itertools
import math
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import limb_bounds as LB  # noqa: E402

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
D = -121665 * pow(121666, P - 2, P) % P
OFF = (0, 26, 51, 77, 102, 128, 153, 179, 204, 230)
WID = (26, 25, 26, 25, 26, 25, 26, 25, 26, 25)
MAX_ITEMS = 20000

# ---- roles: limb-wise inclusive upper bounds ---------------------------------------------------------------------
C = list(LB.CARRIED)                 # output of fe_mul / fe_sq / fe_mul_chain / fe_carry
TABLE = list(LB.TABLE)               # canonical limbs (comb table entries): 2^26 - 1 / 2^25 - 1
P2 = list(LB.P2)                     # 2p limb-wise: -k of a canonical k
ADD = LB.add(C, C)                   # one fe_add of carried values
SUB = LB.sub(C, C, LB.P2)            # one fe_sub of carried values
WIDE = LB.add(SUB, LB.P2)            # fe_eq's difference of a SUB value and a carried one, before fe_is_zero
U31 = [2**31 - 1] * 10               # fe_carry: "inputs < 2^31"
# fe_reduce_par's output, as fe25519.h states it (2^26 + 2^17.6, 2^25 + 2^16.6, then width + 2^13.4), rounded up
PAR = [2**26 + math.ceil(2**17.6), 2**25 + math.ceil(2**16.6)] + \
      [2**WID[i] + math.ceil(2**13.4) for i in range(2, 10)]

SPECIALS = (P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 2**255 - 1, 2**255, 2**255 + 18)


def value(limbs):
    return sum(int(x) << o for x, o in zip(limbs, OFF))


def tight(v):
    """The radix-2^25.5 digits of v; what does not fit below 2^255 stays in limb 9."""
    return [(v >> OFF[i]) & ((1 << WID[i]) - 1) for i in range(9)] + [v >> 230]


def fits(vec, B):
    return all(0 <= x <= b for x, b in zip(vec, B))


def loose(v, B):
    """A non-tight form of v within B: every limb borrows from the limb above as many units as its bound allows."""
    t = tight(v)
    for i in range(9):
        k = min(t[i + 1], (B[i] - t[i]) >> WID[i])
        t[i] += k << WID[i]
        t[i + 1] -= k
    return t


def two_tight(v, B, rnd):
    """v as the limb-wise sum of two tight vectors (what one fe_add leaves), for roles that hold such a sum."""
    a = rnd.randrange(v + 1)
    return [x + y for x, y in zip(tight(a), tight(v - a))]


def structured(B, rnd):
    """The deterministic vectors of role B: (kind, vector)."""
    out = [("max", list(B)), ("max-1", [b - 1 for b in B]), ("zero", [0] * 10),
           ("ones", [(1 << w) - 1 for w in WID])]
    for i in range(10):
        out.append((f"only{i}", [B[j] if j == i else 0 for j in range(10)]))
        out.append((f"without{i}", [0 if j == i else B[j] for j in range(10)]))
    vals = [v for v in SPECIALS if (v >> 230) <= B[9]]
    vals += [k * P for k in range(0, 9) if (k * P >> 230) <= B[9] and k * P not in vals]
    holds_sum = all(2 * ((1 << w) - 1) <= b for w, b in zip(WID, B))
    for v in vals:
        out.append((f"tight({v:#x})", tight(v)))
        out.append((f"loose({v:#x})", loose(v, B)))
        if holds_sum and v < 2**256:
            out.append((f"sum({v:#x})", two_tight(v, B, rnd)))
    for kind, vec in out:
        assert fits(vec, B), (kind, vec, B)
    return out


def mixed(B, rnd):
    return [rnd.choice((0, 1, b - 1, b, rnd.randint(0, b))) for b in B]


def uniform(B, rnd):
    return [rnd.randint(0, b) for b in B]


def small(rnd):
    return [rnd.randint(0, 3) for _ in range(10)]


def operand_cases(roles, rnd, n_mixed, n_uniform, groups=()):
    """Tuples of limb vectors, one per operand of an op whose operands have the bounds `roles`:
    every operand at the same structured kind; each operand in turn through its structured vectors with the
    others small, at their maximum, and random; each group of operands (a chain product's pair) at its extremes
    with the others small; then mixed and uniform random limbs."""
    k = len(roles)
    st = [structured(B, rnd) for B in roles]
    cases = []
    for kind in ("max", "max-1", "zero", "ones") + tuple(f"only{i}" for i in range(10)) + \
            tuple(f"without{i}" for i in range(10)):
        cases.append(tuple(dict(s)[kind] for s in st))
    for j in range(k):
        for _, vec in st[j]:
            for others in ("small", "max", "uniform"):
                row = [small(rnd) if others == "small" else list(B) if others == "max" else uniform(B, rnd)
                       for B in roles]
                row[j] = vec
                cases.append(tuple(row))
    for g in groups:
        for kind in ("max", "max-1", "ones"):
            cases.append(tuple(dict(st[j])[kind] if j in g else small(rnd) for j in range(k)))
    cases += [tuple(mixed(B, rnd) for B in roles) for _ in range(n_mixed)]
    cases += [tuple(uniform(B, rnd) for B in roles) for _ in range(n_uniform)]
    for row in cases:
        for vec, B in zip(row, roles):
            assert fits(vec, B), (vec, B)
    return cases


def rows(cases, extra=None):
    """(n, words) uint32 array of operand tuples; extra: one more word per case."""
    flat = [[x for vec in row for x in vec] + ([extra[i]] if extra is not None else []) for i, row in enumerate(cases)]
    assert 0 < len(flat) <= MAX_ITEMS, len(flat)
    a = np.array(flat, dtype=np.uint64)
    assert (a < 2**32).all()
    return np.ascontiguousarray(a.astype(np.uint32))


def with_signs(cases):
    """Every case under both signs."""
    both = [c for c in cases for _ in (0, 1)]
    return both, [i & 1 for i in range(len(both))]


def _valid_product(f, g):
    LB.mulmax(f, g)  # asserts u32 premultiplies, u64 columns and the carried result (tools/limb_bounds.py)
    return (f, g)


# operand bounds of the products: what the comb step and the doubling feed them (tools/limb_bounds.py), and the
# widest pair the header allows ("any operands produced by one add/sub of carried values")
MUL_ROLES = [_valid_product(SUB, SUB), _valid_product(ADD, ADD), _valid_product(C, P2), _valid_product(C, C)]
SQ_ROLES = [SUB, ADD, C]
for _f in SQ_ROLES:
    LB.mulmax(_f, _f)
MADD = {neg: LB.MADD_PRODUCTS(neg) for neg in (False, True)}
CHAIN_ROLES = {
    1: [[_valid_product(SUB, SUB)], [_valid_product(ADD, ADD)], [_valid_product(C, P2)]],
    # the comb step's three input products (both signs of k) and its output products without T
    3: [[MADD[neg][k] for k in ("a", "b", "c")] for neg in (False, True)] +
       [[MADD[False][k] for k in ("X3", "Y3", "Z3")]],
    4: [[MADD[False][k] for k in ("X3", "Y3", "Z3", "T3")]],
}
for _sets in CHAIN_ROLES.values():
    for _s in _sets:
        for _f, _g in _s:
            _valid_product(_f, _g)


# ---- case sets, one per op (built once, shared by every test that needs them) ---------------------------------------
_cache = {}


def cases(name):
    """The op's input rows, (n, words in) uint32."""
    if name not in _cache:
        _cache[name] = _BUILD[name]()
        assert len(_cache[name]) <= MAX_ITEMS
    return _cache[name]


def _seed(name):
    return random.Random("arith:" + name)


def _mul_cases(name, par):
    rnd = _seed(name)
    out = []
    for f, g in MUL_ROLES + ([(PAR, PAR)] if par else []):
        out += operand_cases([f, g], rnd, 1500, 500)
    return rows(out)


def _sq_cases(name, par):
    rnd = _seed(name)
    out = []
    for f in SQ_ROLES + ([PAR] if par else []):
        out += operand_cases([f], rnd, 2500, 500)
    return rows(out)


def _chain_cases(n):
    rnd = _seed(f"chain{n}")
    out = []
    for pairs in CHAIN_ROLES[n]:
        roles = [b for pair in pairs for b in pair]
        out += operand_cases(roles, rnd, 1500, 500, groups=[(2 * m, 2 * m + 1) for m in range(n)])
    return rows(out)


def _pair_cases(name, role_sets, n_mixed=1500, n_uniform=500):
    rnd = _seed(name)
    out = []
    for roles in role_sets:
        out += operand_cases(list(roles), rnd, n_mixed, n_uniform)
    return rows(out)


def _eq_cases():
    """fe_eq: the general cases (almost all unequal) and pairs of different forms of congruent or adjacent values."""
    rnd = _seed("fe_eq")
    out = []
    for ra, rb in ((SUB, SUB), (C, U31)):
        out += operand_cases([ra, rb], rnd, 800, 200)
        for _, a in structured(ra, rnd) + [("uniform", uniform(ra, rnd)) for _ in range(300)]:
            v = value(a)
            for w in (v % P, v % P + P, v, v % P + 1, (v + P - 1) % P):
                if (w >> 230) <= rb[9]:
                    for b in (tight(w), loose(w, rb)):
                        assert fits(b, rb)
                        out.append((a, b))
    return rows(out)


def _from_words_cases():
    rnd = _seed("fe_from_words")
    vals = list(SPECIALS) + [v + 2**255 for v in SPECIALS if v + 2**255 < 2**256] + [0, 1, 2**256 - 1]
    vals += [1 << k for k in range(256)] + [(2**256 - 1) ^ (1 << k) for k in range(256)]
    vals += [rnd.getrandbits(256) for _ in range(2000)]
    return _words(vals, 8)


def _words(vals, n):
    a = np.array([[(v >> (32 * t)) & 0xFFFFFFFF for t in range(n)] for v in vals], dtype=np.uint32)
    assert 0 < len(a) <= MAX_ITEMS
    return a


def _madd_cases():
    rnd = _seed("ge_madd")
    cs, sign = with_signs(operand_cases([C, C, C, C, TABLE, TABLE, TABLE], rnd, 2500, 1000))
    return rows(cs, sign)


def _from_ab_cases():
    rnd = _seed("ge_from_ab")
    cs, sign = with_signs(operand_cases([TABLE, TABLE, TABLE], rnd, 1500, 500))
    return rows(cs, sign)


def reduce512_values():
    """The value list of test_host_harness.test_reduce512, reused: the test runs against a recorder that answers
    x mod L, so its list is taken as it stands and never copied here."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("host_harness_tests_for_arith_cases",
                                                  os.path.join(ROOT, "tests", "test_host_harness.py"))
    T = importlib.util.module_from_spec(spec)  # (a private copy: the test module itself is left to pytest)
    spec.loader.exec_module(T)

    class Recorder:
        def __init__(self):
            self.seen = []

        def hh_reduce512(self, x64, out32):
            x = int.from_bytes(bytes(x64), "little")
            self.seen.append(x)
            out32.raw = (x % L).to_bytes(32, "little")

    r = Recorder()
    T.test_reduce512(r)
    assert len(r.seen) > 3000
    return r.seen


def _reduce512_cases():
    rnd = _seed("sc_reduce512")
    vals = reduce512_values()
    # extremes of the radix-2^21 fold: every 21-bit limb all ones; only limbs 12..24; only limbs 18..24; x[15] alone
    all_limbs = sum(0x1FFFFF << (21 * i) for i in range(24)) | (0xFF << 504)
    vals += [all_limbs, all_limbs >> 252 << 252, all_limbs >> 378 << 378, 0xFFFFFFFF << 480]
    vals += [(0x1FFFFF << (21 * i)) % 2**512 for i in range(25)] + [(0x100000 << (21 * i)) % 2**512 for i in range(25)]
    # multiples of L +- 1 up to 2^512
    kmax = (2**512 - 1) // L
    ks = sorted({1 << j for j in range(260)} | {(1 << j) - 1 for j in range(1, 261)} | {kmax, kmax - 1} |
                {rnd.randrange(kmax) for _ in range(300)})
    vals += [k * L + d for k in ks if 0 < k <= kmax for d in (-1, 0, 1) if k * L + d < 2**512]
    vals += [rnd.getrandbits(512) for _ in range(3000)]
    assert all(0 <= v < 2**512 for v in vals)
    return _words(vals, 16)


MULADD_EDGES = (0, 1, L - 1, L, 2**252, 2**255 - 1, 2**256 - 1)


def _muladd_cases():
    rnd = _seed("sc_muladd")
    trip = list(itertools.product(MULADD_EDGES, repeat=3))
    trip += [tuple(rnd.getrandbits(256) for _ in range(3)) for _ in range(2000)]
    trip += [tuple(rnd.choice(MULADD_EDGES + (rnd.getrandbits(256),)) for _ in range(3)) for _ in range(1000)]
    return _words([a | (b << 256) | (c << 512) for a, b, c in trip], 24)


def _lt_L_cases():
    rnd = _seed("sc_lt_L")
    vals = [0, 1, L - 2, L - 1, L, L + 1, L + 2, 2**252, 2**252 - 1, 2**253, 2**255, 2**256 - 1, 2 * L, 2 * L - 1]
    for t in range(8):  # one word of L one up / one down / zero / all ones
        w = (L >> (32 * t)) & 0xFFFFFFFF
        for nw in ((w + 1) & 0xFFFFFFFF, (w - 1) & 0xFFFFFFFF, 0, 0xFFFFFFFF):
            vals.append(L & ~(0xFFFFFFFF << (32 * t)) | (nw << (32 * t)))
    vals += [rnd.getrandbits(256) for _ in range(1000)] + [rnd.randrange(2 * L) for _ in range(1000)]
    return _words(vals, 8)


_BUILD = {
    "fe_mul": lambda: _mul_cases("fe_mul", False),
    "fe_sq": lambda: _sq_cases("fe_sq", False),
    "fe_mul_par": lambda: _mul_cases("fe_mul_par", True),
    "fe_sq_par": lambda: _sq_cases("fe_sq_par", True),
    "fe_mul_chain1": lambda: _chain_cases(1),
    "fe_mul_chain3": lambda: _chain_cases(3),
    "fe_mul_chain4": lambda: _chain_cases(4),
    "fe_add": lambda: _pair_cases("fe_add", [(C, C), (PAR, PAR)]),
    "fe_sub": lambda: _pair_cases("fe_sub", [(ADD, C), (PAR, PAR)]),
    "fe_neg": lambda: _pair_cases("fe_neg", [(C,), (PAR,)]),
    "fe_carry": lambda: _pair_cases("fe_carry", [(U31,), (SUB,)]),
    "fe_to_words": lambda: _pair_cases("fe_to_words", [(C,), (WIDE,), (U31,)]),
    "fe_from_words": _from_words_cases,
    "fe_is_zero": lambda: _pair_cases("fe_is_zero", [(C,), (WIDE,), (U31,)]),
    "fe_is_negative": lambda: _pair_cases("fe_is_negative", [(C,), (WIDE,), (U31,)]),
    "fe_eq": _eq_cases,
    # the three forms of the comb step run the same cases (they are compared limb for limb)
    "ge_madd": _madd_cases,
    "ge_madd_chain": lambda: cases("ge_madd"),
    "ge_madd_chain_not": lambda: cases("ge_madd"),
    "ge_from_ab": _from_ab_cases,
    "ge_dbl": lambda: _pair_cases("ge_dbl", [(C, C, C)], 3000, 1000),
    "sc_reduce512": _reduce512_cases,
    "sc_muladd": _muladd_cases,
    "sc_lt_L": _lt_L_cases,
}

GROUPS = {
    "multiply": ("fe_mul", "fe_sq", "fe_mul_par", "fe_sq_par"),
    "chain": ("fe_mul_chain1", "fe_mul_chain3", "fe_mul_chain4"),
    "linear": ("fe_add", "fe_sub", "fe_neg", "fe_carry"),
    "canonical": ("fe_to_words", "fe_from_words", "fe_is_zero", "fe_is_negative", "fe_eq"),
    "comb_step": ("ge_madd", "ge_madd_chain", "ge_madd_chain_not", "ge_from_ab"),
    "doubling": ("ge_dbl",),
    "scalars": ("sc_reduce512", "sc_muladd", "sc_lt_L"),
}
assert sorted(n for g in GROUPS.values() for n in g) == sorted(_BUILD)


# ---- running an op: one hook call per op and backend ----------------------------------------------------------------
def run(backend, name, inp=None):
    """The op's outputs on `inp` (default: its whole case set, one call, kept per backend)."""
    op, win, wout = backend.ops[name]
    whole = inp is None
    if whole:
        if name in backend.results:
            return backend.results[name]
        inp = cases(name)
    assert inp.dtype == np.uint32 and inp.ndim == 2 and inp.shape[1] == win, (name, inp.shape, win)
    out = np.full((len(inp), wout), 0xA5A5A5A5, dtype=np.uint32)
    rc = backend.call(op, np.ascontiguousarray(inp), out, len(inp))
    assert rc == 0, (name, rc)
    if whole:
        backend.results[name] = out
    return out


def read_ops(info):
    """{name: (op, win, wout)} from the hook's info function (int op, char** name, u32* win, u32* wout)."""
    import ctypes
    ops, op = {}, 0
    while True:
        nm, wi, wo = ctypes.c_char_p(), ctypes.c_uint32(), ctypes.c_uint32()
        if info(op, ctypes.byref(nm), ctypes.byref(wi), ctypes.byref(wo)) != 0:
            break
        ops[nm.value.decode()] = (op, wi.value, wo.value)
        op += 1
    return ops


# ---- model and comparisons -------------------------------------------------------------------------------------------
def fes(a):
    """Rows of k*10 limbs -> list of rows of k Python-integer values."""
    a = a.astype(np.uint64).reshape(len(a), -1, 10)
    vals = np.zeros(a.shape[:2], dtype=object)
    for i in range(10):
        vals = vals + (a[:, :, i].astype(object) << OFF[i])
    return vals.tolist()


def ints(a):
    """Rows of 32-bit little-endian words -> Python integers."""
    v = np.zeros(len(a), dtype=object)
    for t in range(a.shape[1]):
        v = v + (a[:, t].astype(object) << (32 * t))
    return v.tolist()


def expect_values(name, got, want):
    """got: (n, k*10) raw limbs; want: n rows of k integers; equal mod p, coordinate by coordinate."""
    g = fes(got)
    bad = [(i, j) for i, (gr, wr) in enumerate(zip(g, want)) for j, (x, y) in enumerate(zip(gr, wr))
           if (x - y) % P != 0]
    assert not bad, (f"{name}: {len(bad)} of {len(g) * len(g[0])} values differ mod p; "
                     f"first (case, coordinate) {bad[:5]}")


def expect_within(name, got, bound):
    """Every raw output limb within the bound vector."""
    limbs = got.reshape(len(got), -1, 10).astype(np.int64)
    over = limbs - np.array(bound, dtype=np.int64)
    bad = np.argwhere(over > 0)
    assert len(bad) == 0, (f"{name}: {len(bad)} limbs over their bound; first (case, coordinate, limb) "
                           f"{bad[:5].tolist()}, largest overshoot per limb {over.max(axis=(0, 1)).tolist()}")


def expect_equal(what, a, b):
    bad = np.argwhere(a != b)
    assert len(bad) == 0, f"{what}: {len(bad)} words differ; first (case, word) {bad[:5].tolist()}"


def expect_words(name, got, want):
    g = ints(got)
    bad = [(i, hex(x), hex(y)) for i, (x, y) in enumerate(zip(g, want)) if x != y]
    assert not bad, f"{name}: {len(bad)} of {len(g)} results differ; first (case, got, want) {bad[:3]}"


def madd_model(row, neg):
    X, Y, Z, T, qa, qb, k = row
    a, b, c = (Y - X) * qa, (Y + X) * qb, T * (-k if neg else k)
    E, F, G, H = b - a, Z - c, Z + c, b + a
    return [E * F, G * H, F * G, E * H]


def dbl_model(row):
    X, Y, Z = row
    A, B, C2, t = X * X, Y * Y, 2 * Z * Z, (X + Y) ** 2
    H = A + B
    E, G = H - t, A - B
    F = C2 + G
    return [E * F, G * H, F * G, E * H]


def check_multiply(be):
    for name, bound in (("fe_mul", C), ("fe_mul_par", PAR)):
        got = run(be, name)
        expect_values(name, got, [[f * g] for f, g in fes(cases(name))])
        expect_within(name, got, bound)
    for name, bound in (("fe_sq", C), ("fe_sq_par", PAR)):
        got = run(be, name)
        expect_values(name, got, [[f * f] for f, in fes(cases(name))])
        expect_within(name, got, bound)


def check_chain(be):
    for n in (1, 3, 4):
        name = f"fe_mul_chain{n}"
        inp, got = cases(name), run(be, name)
        expect_values(name, got, [[r[2 * m] * r[2 * m + 1] for m in range(n)] for r in fes(inp)])
        expect_within(name, got, C)
        # "identical outputs and bounds": limb for limb what fe_mul gives on each of the N operand pairs
        single = run(be, "fe_mul", np.ascontiguousarray(inp.reshape(-1, 20)))
        expect_equal(f"{name} against fe_mul", got.reshape(-1, 10), single)


def check_linear(be):
    inp, got = cases("fe_add"), run(be, "fe_add")
    expect_values("fe_add", got, [[f + g] for f, g in fes(inp)])
    expect_equal("fe_add limbs (no carry, no wrap)", got.astype(np.int64), inp[:, :10].astype(np.int64) + inp[:, 10:])
    inp, got = cases("fe_sub"), run(be, "fe_sub")
    expect_values("fe_sub", got, [[f - g] for f, g in fes(inp)])
    expect_equal("fe_sub limbs (f + 2p - g, no wrap)", got.astype(np.int64),
                 inp[:, :10].astype(np.int64) + np.array(P2, dtype=np.int64) - inp[:, 10:])
    inp, got = cases("fe_neg"), run(be, "fe_neg")
    expect_values("fe_neg", got, [[-f] for f, in fes(inp)])
    expect_within("fe_neg", got, P2)
    inp, got = cases("fe_carry"), run(be, "fe_carry")
    expect_values("fe_carry", got, fes(inp))
    expect_within("fe_carry", got, C)


def check_canonical(be):
    for name in ("fe_to_words", "fe_is_zero", "fe_is_negative"):
        vals = [v % P for v, in fes(cases(name))]
        want = vals if name == "fe_to_words" else [int(v == 0) for v in vals] if name == "fe_is_zero" else \
            [v & 1 for v in vals]
        expect_words(name, run(be, name), want)
    inp, got = cases("fe_from_words"), run(be, "fe_from_words")
    want = [x % 2**255 for x in ints(inp)]  # bit 255 ignored, the value NOT reduced
    g = [v for v, in fes(got)]
    bad = [(i, hex(x), hex(y)) for i, (x, y) in enumerate(zip(g, want)) if x != y]
    assert not bad, f"fe_from_words: {len(bad)} differ; first {bad[:3]}"
    expect_within("fe_from_words", got, TABLE)
    pairs = fes(cases("fe_eq"))
    want = [int((a - b) % P == 0) for a, b in pairs]
    assert 500 < sum(want) < len(want) - 500  # both answers are well represented
    expect_words("fe_eq", run(be, "fe_eq"), want)


def check_comb_step(be):
    inp = cases("ge_madd")
    want = [madd_model(r, s & 1) for r, s in zip(fes(inp[:, :70]), inp[:, 70].tolist())]
    plain, chain, chain_not = run(be, "ge_madd"), run(be, "ge_madd_chain"), run(be, "ge_madd_chain_not")
    for name, got, k in (("ge_madd", plain, 4), ("ge_madd_chain", chain, 4), ("ge_madd_chain_not", chain_not, 3)):
        expect_values(name, got, [w[:k] for w in want])
        expect_within(name, got, C)
    expect_equal("ge_madd_ab<true, true> against <true, false>", chain, plain)
    expect_equal("ge_madd_ab<false, true> against <true, false> on X, Y, Z", chain_not, plain[:, :30])
    inp, got = cases("ge_from_ab"), run(be, "ge_from_ab")
    dinv = pow(D, P - 2, P)
    want = [[qb - qa, qa + qb, 1, (-k if s & 1 else k) * dinv]
            for (qa, qb, k), s in zip(fes(inp[:, :30]), inp[:, 30].tolist())]
    expect_values("ge_from_ab", got, want)
    expect_within("ge_from_ab", got, C)


def check_doubling(be):
    got = run(be, "ge_dbl")
    expect_values("ge_dbl", got, [dbl_model(r) for r in fes(cases("ge_dbl"))])
    expect_within("ge_dbl", got, C)


def check_scalars(be):
    expect_words("sc_reduce512", run(be, "sc_reduce512"), [x % L for x in ints(cases("sc_reduce512"))])
    m = (1 << 256) - 1
    expect_words("sc_muladd", run(be, "sc_muladd"),
                 [((x & m) * ((x >> 256) & m) + (x >> 512)) % L for x in ints(cases("sc_muladd"))])
    expect_words("sc_lt_L", run(be, "sc_lt_L"), [int(x < L) for x in ints(cases("sc_lt_L"))])


CHECKS = {"multiply": check_multiply, "chain": check_chain, "linear": check_linear, "canonical": check_canonical,
          "comb_step": check_comb_step, "doubling": check_doubling, "scalars": check_scalars}
assert sorted(CHECKS) == sorted(GROUPS)


def check_all_maximum_everywhere():
    """Every op that takes limb vectors has the case with every limb of every operand at its role's maximum."""
    tops = {"fe_mul": SUB + SUB, "fe_sq": SUB, "fe_mul_par": SUB + SUB, "fe_sq_par": SUB, "fe_mul_chain1": SUB + SUB,
            "fe_mul_chain3": [x for pair in CHAIN_ROLES[3][1] for b in pair for x in b],
            "fe_mul_chain4": [x for pair in CHAIN_ROLES[4][0] for b in pair for x in b],
            "fe_add": C + C, "fe_sub": ADD + C, "fe_neg": C, "fe_carry": U31, "fe_to_words": WIDE, "fe_is_zero": WIDE,
            "fe_is_negative": WIDE, "fe_eq": SUB + SUB, "ge_madd": C * 4 + TABLE * 3 + [1],
            "ge_madd_chain": C * 4 + TABLE * 3 + [0], "ge_madd_chain_not": C * 4 + TABLE * 3 + [1],
            "ge_from_ab": TABLE * 3 + [1], "ge_dbl": C * 3}
    for name, top in tops.items():
        hit = (cases(name) == np.array(top, dtype=np.uint32)).all(axis=1)
        assert hit.any(), name


def check_hook_edges(be):
    """n = 1, 63, 64, 65 answer as the same items do inside the large call; bad arguments are refused and nothing
    is written."""
    for name in ("fe_mul_chain3", "ge_madd_chain", "fe_to_words", "sc_reduce512"):
        whole = run(be, name)
        for n in (1, 63, 64, 65):
            for start in (0, len(whole) - n):
                part = run(be, name, cases(name)[start:start + n])
                expect_equal(f"{name} n={n} from {start}", part, whole[start:start + n])
    op, win, wout = be.ops["fe_mul"]
    inp = cases("fe_mul")[:4]
    out = np.full((4, wout), 0xA5A5A5A5, dtype=np.uint32)
    nops = len(be.ops)
    assert sorted(o for o, _, _ in be.ops.values()) == list(range(nops))
    for args in ((op, None, out, 4), (op, inp, None, 4), (-1, inp, out, 4), (nops, inp, out, 4), (1 << 30, inp, out, 4),
                 (op, inp, out, 0), (op, inp, out, (1 << 20) + 1)):
        assert be.call(*args) < 0, (args[0], args[3])
        assert (out == 0xA5A5A5A5).all()
    assert be.call(op, inp, out, 4) == 0 and not (out == 0xA5A5A5A5).all()
