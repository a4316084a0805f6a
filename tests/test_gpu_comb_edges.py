"""GPU: the edge-digit fixture (tests/golden/comb_edges.npz) through every comb kernel form of every key plan.

The fixture's rows put digits 0, +-1 and +-2^(w-1) (and their neighbours) at every position of the base-point plan
and of the four key plans -- table entries and sign cases a random round reaches about once in 2^25 signatures --
and follow each with a twin one unit away that must be rejected.  launch_comb_plan picks among the latency kernel
(8 or 4 lanes per signature), the pair kernel, comb_kernel<85> and its three chain forms (4 waves, 8 waves with
paired priorities, falling priorities); each is forced in turn for each key plan, so that every instantiation reads
those entries, the 32-position plan's 64-bit sign mask included.  Expected bits are the fixture's (both CPU oracles,
tests/test_comb_edges.py), never the GPU library's.  The signing kernels get envelopes whose nonce has the edge
digits, against the C oracle's signer."""
import ctypes
import os

import numpy as np
import pytest

import comb_edges as ce
from conftest import ROOT, golden_batches
from test_gpu_verify import gv, verify  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
BIG = 1_000_000_000
CHAIN_N = 65536 + 77   # PBFT_CHAIN_MIN_N (the chain forms exist from there) and a partial last wave

# form -> ((option, value) ..., N or None for the fixture as it is)
FORMS = {
    "latency8": ((("OPT_SPLIT_BELOW", BIG), ("OPT_LAT_SPLIT", 8)), None),
    "latency4": ((("OPT_SPLIT_BELOW", BIG), ("OPT_LAT_SPLIT", 4)), None),
    "pair": ((("OPT_SPLIT_BELOW", 0), ("OPT_COMB_PAIR", 1)), None),
    "comb85": ((("OPT_SPLIT_BELOW", 0), ("OPT_COMB_PAIR", 0)), None),
    "chain4": ((("OPT_SPLIT_BELOW", 0), ("OPT_COMB_PAIR", 0), ("OPT_COMB_PRIO", 0), ("OPT_COMB_BALANCE", 0)), CHAIN_N),
    "chain8prio": ((("OPT_SPLIT_BELOW", 0), ("OPT_COMB_PAIR", 0), ("OPT_COMB_PRIO", 1)), CHAIN_N),
    "chainbal": ((("OPT_SPLIT_BELOW", 0), ("OPT_COMB_PAIR", 0), ("OPT_COMB_PRIO", 0), ("OPT_COMB_BALANCE", 1)), CHAIN_N),
}
# one key: 671 MB of tables under the 13-position plan, 268 MB (14), 63 MB (16), 0.5 MB (32)
PLANS = [(0, 13), (400, 14), (100, 16), (10, 32)]


@pytest.fixture(scope="module")
def fx():
    return ce.load()


@pytest.fixture(scope="module")
def tiled(fx):
    return ce.tile(fx, CHAIN_N)


def mismatch(fx, got, bm, exp, rows, what):
    """None, or what differs: the (plan, position, target, row kind) tags of the first wrong bits."""
    n = len(exp)
    bad = np.nonzero(got != exp)[0]
    if len(bad):
        return (what, f"{len(bad)} of {n} bits differ", ce.describe(fx, rows[bad[:12]]))
    if len(bm) != (n + 63) // 64 or (n % 64 and int(bm[-1]) >> (n % 64)):
        return (what, "bitmap length or bits past N")
    return None


def set_options(v, opts):
    for name, value in opts:
        v.set_option(getattr(v, name), value)


def restore_options(v):
    set_options(v, (("OPT_LAT_SPLIT", 0), ("OPT_COMB_PAIR", 2), ("OPT_COMB_PRIO", 2), ("OPT_COMB_BALANCE", 2)))


@pytest.mark.parametrize("budget_mb,pa", PLANS)
def test_edge_rows_every_kernel_form(gv, fx, tiled, budget_mb, pa):  # noqa: F811
    v = gv.clone()   # (the forced threshold and budget go away with the clone)
    try:
        if budget_mb:
            v.set_option(v.OPT_KEY_TABLE_BUDGET_MB, budget_mb)
        assert v.set_keys(fx["key"].reshape(1, 32)).all()
        assert v.positions() == (ce.PLAN_B[0], pa)
        rows = np.arange(len(fx["S"]))
        failures = []
        for form, (opts, n) in FORMS.items():
            try:
                set_options(v, opts)
                if n is None:
                    R, S, M, exp, idx = fx["R"], fx["S"], fx["msg"], fx["expected"].astype(bool), rows
                else:
                    R, S, M, exp, idx = tiled
                got, bm = verify(v, R, S, np.zeros(len(R), np.uint16), M, 85)
                failures.append(mismatch(fx, got, bm, exp, idx, (pa, form)))
            finally:
                restore_options(v)
        failures = [f for f in failures if f]
        # (every form is run, so a report names each form that is wrong)
        assert not failures, "\n".join(str(f) for f in failures)
    finally:
        v.close()


def test_edge_rows_votes_form(gv, fx, tiled):  # noqa: F811
    """pbft_verify_votes with the default kernel selection (13-position key plan), at both sizes."""
    from pbft_amd import bitmap_to_bool
    v = gv.clone()
    try:
        assert v.set_keys(fx["key"].reshape(1, 32)).all() and v.positions()[1] == 13
        env, inv = np.unique(fx["msg"], axis=0, return_inverse=True)
        inv = inv.reshape(-1).astype(np.uint32)
        rows = np.arange(len(fx["S"]))
        for R, S, M, exp, idx in ((fx["R"], fx["S"], fx["msg"], fx["expected"].astype(bool), rows), tiled):
            ei = inv[idx]
            assert (env[ei] == M).all()
            bm = v.verify_votes(R, S, np.zeros(len(R), np.uint16), ei, env)
            m = mismatch(fx, bitmap_to_bool(bm, len(R)), bm, exp, idx, ("votes", len(R)))
            assert m is None, m
    finally:
        v.close()


@pytest.mark.parametrize("budget_mb,pa", [(0, 13), (40, 32)])
def test_golden_corpus_three_kernels(gv, golden, budget_mb, pa):  # noqa: F811
    """comb_latency_kernel, comb_pair_kernel and comb_kernel (<85> for the envelope length, <-1> at every other one:
    every SHA-512 padding edge of the golden corpus) give the expected bits of every golden batch, under the default
    key plan and under the 32-position one, whose 42 steps take the 64-bit sign mask.  With PBFT_OPT_SPLIT_BELOW = 0
    alone a batch this small runs comb_pair_kernel by size (test_gpu_verify.py's
    test_latency_mode_split_kernel_matches_single_lane compares the latency kernel with that one); comb_kernel needs
    the pair form forced off as well."""
    v = gv.clone()
    try:
        if budget_mb:
            v.set_option(v.OPT_KEY_TABLE_BUDGET_MB, budget_mb)
        for leg, opts in (("latency", (("OPT_SPLIT_BELOW", BIG),)),
                          ("pair", (("OPT_SPLIT_BELOW", 0), ("OPT_COMB_PAIR", 1))),
                          ("comb", (("OPT_SPLIT_BELOW", 0), ("OPT_COMB_PAIR", 0)))):
            set_options(v, opts)
            for ml, b in golden_batches(golden):
                assert (v.set_keys(b["keys"]) == b["key_ok"].astype(bool)).all()
                assert v.positions()[1] == pa
                got, _ = verify(v, b["R"], b["S"], b["key_idx"], b["msg"], ml)
                bad = np.nonzero(got != b["expected"].astype(bool))[0]
                assert len(bad) == 0, (pa, leg, ml, bad[:10], b["cls"][bad[:10]])
    finally:
        v.close()


@pytest.fixture(scope="module")
def oracle_sigs(fx):
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))
    vp = ctypes.c_void_p
    lib.oracle_sign_batch.argtypes = [vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, vp, vp,
                                      ctypes.c_int]
    lib.oracle_public_key.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    n = len(fx["sg_msg"])
    seeds = np.ascontiguousarray(fx["sg_seed"].reshape(1, 32))
    idx = np.zeros(n, np.uint16)
    buf = np.zeros(n * 85 + 16, np.uint8)
    buf[: n * 85] = fx["sg_msg"].reshape(-1)
    oR, oS = np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8)
    assert lib.oracle_sign_batch(seeds.ctypes.data, idx.ctypes.data, buf.ctypes.data, 85, 85, n, oR.ctypes.data,
                                 oS.ctypes.data, 4) == 0
    pk = ctypes.create_string_buffer(32)
    lib.oracle_public_key(pk, fx["sg_seed"].tobytes())
    assert (oR == fx["sg_R"]).all() and (oS == fx["sg_S"]).all() and pk.raw == fx["sg_pub"].tobytes()
    return oR, oS, pk.raw


def tags(fx, bad):
    return [(int(fx["sg_pos"][i]), int(fx["sg_target"][i])) for i in bad]


def test_sign_edge_nonces(gv, fx, oracle_sigs):  # noqa: F811
    """pbft_sign_batch on envelopes whose nonce r reads the identity or the last entry of a base-table position."""
    oR, oS, pk = oracle_sigs
    n = len(oR)
    R, S, pub = gv.sign(fx["sg_seed"].reshape(1, 32), np.zeros(n, np.uint16), fx["sg_msg"], 85)
    assert pub[0].tobytes() == pk
    bad = np.nonzero((R != oR).any(axis=1) | (S != oS).any(axis=1))[0]
    assert len(bad) == 0, ("(position, nonce digit) of the signatures that differ:", tags(fx, bad))


def test_egress_signer_edge_nonces(gv, fx, oracle_sigs):  # noqa: F811
    """pbft_sign_votes_frames (the egress signer) on the same envelopes: the 64 signature bytes."""
    oR, oS, pk = oracle_sigs
    v = gv.clone()
    try:
        assert v.set_signing_seed(fx["sg_seed"].tobytes(), 3).tobytes() == pk
        _, off, sigs = v.sign_votes_frames(fx["sg_msg"])
        assert len(off) == len(oR) + 1
        bad = np.nonzero((sigs[:, :32] != oR).any(axis=1) | (sigs[:, 32:] != oS).any(axis=1))[0]
        assert len(bad) == 0, ("(position, nonce digit) of the signatures that differ:", tags(fx, bad))
    finally:
        v.close()
