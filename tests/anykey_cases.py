"""Cases shared by tests/test_anykey.py (the host build) and tests/test_gpu_anykey.py (the gfx950 build): the golden corpus
with every signature's key carried inline, and the (s, k, A) triples of the point hook with their expected encodings
from oracle/ed25519_ref.py.  Computed once per process."""
import functools
import json
import os

import numpy as np

import ed25519_ref as ref
from conftest import GOLDEN, golden_batches

L = ref.L
KAT = json.load(open(os.path.join(GOLDEN, "kat.json")))
NIB8 = int("8" * 64, 16)

# k: small values round the digit edges; every nibble 8 (a carry through all 64 digits); every nibble 7 (no carry at
# all); all ones below 2^252; 2^252 (the top digit alone); L - 1; 2^252 + 2^251 (top digits 1, 8 -> 2, -8)
K_LIST = [0, 1, 7, 8, 9, 15, 16, NIB8 % (1 << 252), int("7" * 63, 16), (1 << 252) - 1, 1 << 252, L - 1,
          (1 << 252) + (1 << 251)]
S_LIST = [0, 1, L - 1]


def recode(k):
    """The 64 signed 4-bit digits of k < 2^253, least significant first: digits 0..62 in [-8, 8), the top one as it
    comes out (anykey_core.h ak_recode), so that k = sum d_i 16^i."""
    ds, c = [], 0
    for i in range(64):
        d = ((k >> (4 * i)) & 15) + c
        c = 1 if (d >= 8 and i < 63) else 0
        ds.append(d - 16 * c)
    assert sum(d << (4 * i) for i, d in enumerate(ds)) == k
    return ds


def _b(x):
    return int(x).to_bytes(32, "little")


@functools.lru_cache(maxsize=None)
def golden_mixed_key():
    g = np.load(os.path.join(GOLDEN, "verify_vectors.npz"))
    for _, b in golden_batches(g):
        rows = np.nonzero(b["cls"] == 10)[0]
        if len(rows):
            return b["keys"][int(b["key_idx"][rows[0]])].tobytes()
    raise AssertionError("no mixed-order key in the golden corpus")


@functools.lru_cache(maxsize=None)
def point_cases():
    """(s [n][32], k [n][32], A [n][32], enc [n][32], key_ok [n], decodes [n]) as uint8 arrays.  enc of a key that does
    not decode is not defined (decodes = 0): only its key_ok is compared."""
    ordinary = bytes.fromhex(KAT["rfc8032"][0]["public"])
    base = ref.compress(ref.BASE)
    special = [base] + [bytes.fromhex(h) for h in KAT["small_order_encodings"]] + \
              [bytes.fromhex(h) for h in KAT["noncanonical_decodable_encodings"]] + [golden_mixed_key()]
    assert len(set(KAT["small_order_encodings"])) >= 8
    triples = [(s, k, ordinary) for k in K_LIST for s in S_LIST]
    j = 0
    for key in special:  # every special key under three (s, k) pairs, walking both lists
        for _ in range(3):
            triples.append((S_LIST[j % 3], K_LIST[(j * 5 + j // 3) % len(K_LIST)], key))
            j += 1
    # each nibble value at window 0 and at window 62, the highest a full-range digit reaches (digits -8 .. 7 there)
    triples += [(1, n, ordinary) for n in range(16)] + [(1, n << 248, ordinary) for n in range(16)]
    rng = np.random.default_rng(20261021)
    for i in range(20):
        k = int.from_bytes(rng.bytes(32), "little") % L
        s = int.from_bytes(rng.bytes(32), "little") % L
        triples.append((s, k, ref.public_key(rng.bytes(32))))
    triples.append((1, 9, (2).to_bytes(32, "little")))  # y = 2: not on the curve
    enc, kok, dec = [], [], []
    sB = {s: ref.pt_mul(s, ref.BASE) for s in S_LIST}
    for s, k, key in triples:
        a = ref.decompress(key)
        dec.append(a is not None)
        kok.append(a is not None and not ref.is_small_order(a))
        if a is None:
            enc.append(bytes(32))
            continue
        sb = sB[s] if s in sB else ref.pt_mul(s, ref.BASE)
        enc.append(ref.compress(ref.pt_add(sb, ref.pt_mul(k, ref.pt_neg(a)))))
    arr = lambda rows: np.frombuffer(b"".join(rows), np.uint8).reshape(-1, 32).copy()  # noqa: E731
    return (arr([_b(t[0]) for t in triples]), arr([_b(t[1]) for t in triples]), arr([t[2] for t in triples]), arr(enc),
            np.array(kok, np.uint8), np.array(dec, np.uint8))


def check_digit_coverage():
    """A property of the inputs: every digit value -8 .. 7 occurs at position 0 and at the highest position it can
    reach (62: the one below the top window), and the top window takes each of its values 0, 1, 2."""
    ks = [int.from_bytes(r.tobytes(), "little") for r in point_cases()[1]]
    ks = [k for k in ks if k < (1 << 253)]
    digs = [recode(k) for k in ks]
    for d in digs:
        assert all(-8 <= x < 8 for x in d[:63]) and 0 <= d[63] <= 2
    at0 = {d[0] for d in digs}
    at62 = {d[62] for d in digs}
    top = {d[63] for d in digs}
    return at0, at62, top


@functools.lru_cache(maxsize=None)
def golden_inline():
    """[(msg_len, R, S, A, msg, expected)] of the 11 golden batches with A[i] = keys[key_idx[i]]."""
    g = np.load(os.path.join(GOLDEN, "verify_vectors.npz"))
    out = []
    for ml, b in golden_batches(g):
        A = np.ascontiguousarray(b["keys"][b["key_idx"]])
        out.append((ml, np.ascontiguousarray(b["R"]), np.ascontiguousarray(b["S"]), A, np.ascontiguousarray(b["msg"]),
                    b["expected"].astype(bool)))
    return out
