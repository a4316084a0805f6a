"""The blocking signing forms pbft_sign_votes_frames, pbft_sign_preprepares_frames and pbft_sign_replies through their C
entry points with the optional outputs null and then each given on its own, and the three forms in turn on one context,
each call larger or smaller than the one before.  The inputs and references are those of test_gpu_egress.py,
test_gpu_propose.py and test_gpu_reply.py (computed once, shared through their caches), each under its module's seed."""
import ctypes
import os

import numpy as np
import pytest

import egress_sim as E
import propose_sim as P
import reply_sim as R
import test_gpu_egress as TE
import test_gpu_propose as TP
import test_gpu_reply as TR
from conftest import ROOT
from pbft_amd import wire
from test_gpu_verify import gv  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
POISON, GUARD = 0xA5, 512
NO_OFF = 2**64 - 1  # the poison of an offsets array


@pytest.fixture(scope="module")
def orc():
    o = ctypes.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))
    o.oracle_public_key.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    return E.bind_oracle(o)


@pytest.fixture(scope="module")
def L():
    return R.bind(wire.load())


@pytest.fixture
def signer(gv):  # noqa: F811
    """install(seed) -> the module's verifier signing as replica 2 under that seed; no seed is left behind."""
    def install(seed):
        gv.set_signing_seed(seed, 2)
        return gv
    yield install
    gv.set_signing_seed(None)


def call_items(fn, v, req, numbers, total, want=()):
    """pbft_sign_preprepares_frames or pbft_sign_replies (`fn`; `numbers` = view[, first_seq]) through the C entry point
    with only the optional outputs named in `want` given, the others null -> (stream, {name: array}); the return code,
    *len and the bytes behind the stream are checked here."""
    data, nbytes, off, ln, ts, cl = req
    n = len(ln)
    out = np.full(total + GUARD, POISON, np.uint8)
    opt = dict(off=np.full(n + 1, NO_OFF, np.uint64), dig=np.full((n, 64), POISON, np.uint8),
               sig=np.full((n, 64), POISON, np.uint8), st=np.full(n, POISON, np.uint8))
    p = {k: (a.ctypes.data if k in want else None) for k, a in opt.items()}
    need = ctypes.c_size_t()
    rc = fn(v._ctx, data.ctypes.data, nbytes, off.ctypes.data, ln.ctypes.data, ts.ctypes.data, cl.ctypes.data, *numbers,
            n, out.ctypes.data, total, ctypes.byref(need), p["off"], p["dig"], p["sig"], p["st"])
    assert rc == 0 and need.value == total, (want, rc, need.value)
    assert (out[total:] == POISON).all(), "bytes behind the stream overwritten"
    return out[:total], opt


def check_items(fn, v, req, numbers, stream, ref):
    """All four optional outputs null, then each alone: the stream and the given output are the reference's, the others
    are not written."""
    got, _ = call_items(fn, v, req, numbers, len(stream))
    assert (got == stream).all()
    for k in ref:
        got, opt = call_items(fn, v, req, numbers, len(stream), want=(k,))
        assert (got == stream).all(), k
        assert (opt[k].reshape(-1) == np.asarray(ref[k]).reshape(-1)).all(), k
        assert all((a == (NO_OFF if j == "off" else POISON)).all() for j, a in opt.items() if j != k), k


@pytest.mark.parametrize("case", ["mixed_7", "mixed_65", "canonical_70"])
def test_proposals_optional_outputs_null(signer, orc, case):
    """With general requests the host's merge reads digests and signatures from its own temporaries."""
    v = signer(TP.SEED)
    if case == "canonical_70":
        if case not in TP._ref:
            TP._ref[case] = P.reference(orc, TP.SEED, 2, 1, 1, [b"testOperation"] * 70, list(range(70)),
                                        ["127.0.0.1:8080"] * 70)
        req, stream, off, dig, sig, st = TP._ref[case]
        numbers = (1, 1)
        assert (st == 0).all()
    else:
        r = TP.reference(orc, *{"mixed_7": (7, 5), "mixed_65": (65, 4)}[case])
        req, stream, off, dig, sig, st = (r[k] for k in ("req", "stream", "off", "dig", "sig", "st"))
        numbers = (TP.VIEW, TP.FIRST)
        assert 0 < int((st == 1).sum()) < len(st)  # general requests among canonical ones
    check_items(v._lib.pbft_sign_preprepares_frames, v, req, numbers, stream, dict(off=off, dig=dig, sig=sig, st=st))


@pytest.mark.parametrize("n,salt,general", [(7, 5, True), (65, 4, True), (70, 6, False)])
def test_replies_optional_outputs_null(signer, orc, L, n, salt, general):
    """With general results the host's merge reads the signatures from its own temporary."""
    v = signer(TR.SEED)
    r = TR.reference(L, orc, n, salt, general=general)
    assert (0 < int((r["st"] == 1).sum()) < n) if general else (r["st"] == 0).all()
    check_items(v._lib.pbft_sign_replies, v, r["req"], (TR.VIEW,), r["stream"],
                {k: r[k] for k in ("off", "dig", "sig", "st")})


@pytest.mark.parametrize("n", [1, 65, 130])
def test_votes_optional_outputs_null(signer, orc, n):
    """frame_off and sigs both null, then each alone."""
    v = signer(TE.SEED)
    env, stream, frame_off, sigs = TE.reference(orc, n, 2)
    rows = np.ascontiguousarray(env, dtype=np.uint8).reshape(-1)
    for want in ((), ("off",), ("sig",)):
        out = np.full(len(stream) + GUARD, POISON, np.uint8)
        off, sig = np.full(n + 1, NO_OFF, np.uint64), np.full((n, 64), POISON, np.uint8)
        need = ctypes.c_size_t()
        rc = v._lib.pbft_sign_votes_frames(v._ctx, rows.ctypes.data, 85, n, out.ctypes.data, len(stream),
                                           ctypes.byref(need), off.ctypes.data if "off" in want else None,
                                           sig.ctypes.data if "sig" in want else None)
        assert rc == 0 and need.value == len(stream), (want, rc)
        assert (out[:len(stream)] == stream).all() and (out[len(stream):] == POISON).all(), want
        assert (off == frame_off).all() if "off" in want else (off == NO_OFF).all(), want
        assert (sig == sigs).all() if "sig" in want else (sig == POISON).all(), want


def test_blocking_forms_in_turn_on_one_context(gv, orc, L):  # noqa: F811
    """On one fresh clone under one seed: replies (7), proposals (130), votes (193), replies (130), proposals (7) -- the
    device staging the calls need grows twice and is then needed smaller, by another form each time.  Every result is
    its reference's."""
    seed = TR.SEED
    key = "in_turn"
    if key not in TR._ref:
        env = TE.make_env(193)
        TR._ref[key] = dict(votes=(env,) + E.oracle_frames(orc, seed, 2, env),
                            pp={n: P.reference(orc, seed, 2, TP.VIEW, TP.FIRST, *P.mixed_ops(n, salt))
                                for n, salt in ((130, 0), (7, 5))})
    want = TR._ref[key]
    c = gv.clone()
    try:
        c.set_signing_seed(seed, 2)

        def replies(n, salt):
            r = TR.reference(L, orc, n, salt)
            stream, off, dig, sig, st = c.sign_replies(TR.VIEW, r["req"])
            assert len(stream) == len(r["stream"]) and (stream == r["stream"]).all(), n
            assert (off == r["off"]).all() and (dig == r["dig"]).all() and (sig == r["sig"]).all(), n
            assert (st == r["st"]).all(), n

        def proposals(n):
            req, stream, off, dig, sig, st = want["pp"][n]
            got = c.sign_preprepares_frames(TP.VIEW, TP.FIRST, req)
            assert len(got[0]) == len(stream) and (got[0] == stream).all(), n
            assert (got[1] == off).all() and (got[2] == dig).all() and (got[3] == sig).all() and (got[4] == st).all(), n

        replies(7, 5)
        proposals(130)
        env, stream, frame_off, sigs = want["votes"]
        got = c.sign_votes_frames(env)
        assert len(got[0]) == len(stream) and (got[0] == stream).all()
        assert (got[1] == frame_off).all() and (got[2] == sigs).all()
        replies(130, 0)
        proposals(7)
    finally:
        c.close()
