"""Shared model behind the edge-digit fixture tests/golden/comb_edges.npz (generator, CPU test and GPU test).

The comb kernels recode a scalar into one signed digit per table position (verify_core.h `digits`): position i of
plan<P, W, NB> is a window of width(i) = W + 1 (i < NB) or W bits; every position but the last yields a digit in
[-2^(w-1), 2^(w-1)) and carries into the next, the last one yields its window plus the carry unrecoded.  A digit d
reads table entry |d| of its position (entry 0 = identity, last entry 2^(w-1)) and negates it for d < 0.

A uniformly random scalar puts a given digit value at a 25- or 26-bit position once in 2^25 or 2^26 tries, so the
fixture holds real signatures searched for those values: per plan and position the digits in `targets()`.
"""
import os

import numpy as np

L = 2**252 + 27742317777372353535851937790883648493
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "comb_edges.npz")

# (P, W, NB) of verify_kernels.h: PLB (base point) and the four key plans, by their position count
PLAN_B = (10, 25, 4)
KEY_PLANS = {13: (13, 19, 7), 14: (14, 18, 2), 16: (16, 15, 14), 32: (32, 7, 30)}
# plan ids as stored in the fixture's `plan` column: 0 = base table (digits of s), else the key plan (digits of k)
PLANS = {0: PLAN_B, **KEY_PLANS}
COUNTS = {0: 56, 13: 74, 14: 80, 16: 92, 32: 188}
SIGNER_COUNT = 19


def width(plan, pos):
    p, w, nb = plan
    return w + 1 if pos < nb else w


def bitoff(plan, pos):
    p, w, nb = plan
    return pos * (w + 1) if pos <= nb else nb * (w + 1) + (pos - nb) * w


def recode(x, plan):
    """The digits of scalar x under `plan`, position 0 first: `digits::take<w>` per position, `take_last` at the top."""
    assert 0 <= x < 1 << 253
    p = plan[0]
    out, carry = [], 0
    for pos in range(p):
        w = width(plan, pos)
        d = (x & ((1 << w) - 1)) + carry
        x >>= w
        if pos < p - 1:
            carry = 1 if d >= 1 << (w - 1) else 0
            d -= carry << w
        out.append(d)
    assert x == 0
    return out


def targets(plan, pos):
    """The edge digits of one position: entries 0, 1, the last entry and its neighbour, both signs where they exist."""
    if pos == plan[0] - 1:
        return [0, 1]  # the top window of a scalar below L reaches no other edge
    h = 1 << (width(plan, pos) - 1)
    return [0, 1, -1, h - 1, -h, -h + 1]


def signer_targets(pos):
    """Nonce digits for the signing kernels (base table): identity and the last entry; identity alone at the top."""
    if pos == PLAN_B[0] - 1:
        return [0]
    return [0, -(1 << (width(PLAN_B, pos) - 1))]


def all_targets(plan_id):
    plan = PLANS[plan_id]
    return [(plan_id, pos, t) for pos in range(plan[0]) for t in targets(plan, pos)]


def envelope(kind, view, seq, digest):
    return b"PBFT" + bytes([kind]) + view.to_bytes(8, "little") + seq.to_bytes(8, "little") + digest


def load():
    """The fixture as a dict of arrays (see gen_comb_edges.py for the columns)."""
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def tile(fx, n):
    """n rows cycling through the fixture: (R, S, msg, expected, row index).  The fixture's length is no multiple of
    64, so every repetition puts a row into another lane."""
    rows = len(fx["S"])
    assert rows % 64
    idx = np.arange(n) % rows
    return fx["R"][idx], fx["S"][idx], fx["msg"][idx], fx["expected"][idx].astype(bool), idx


def describe(fx, rows):
    """The (plan, position, target, twin) tags of fixture rows, for failure messages."""
    return [(int(fx["plan"][r]), int(fx["pos"][r]), int(fx["target"][r]), "twin" if fx["twin"][r] else "valid")
            for r in rows]
