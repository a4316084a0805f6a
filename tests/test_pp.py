"""The canonical-PrePrepare rule and the replica's head path, without a GPU.

The rule (pbft_amd/csrc/wire_pp_core.h) is built for the host into a stand-alone program (tests/native/pp_main.cpp)
under AddressSanitizer + UndefinedBehaviorSanitizer and compared with pbft_wire_decode_json over tests/pp_traffic.py's
corpus, in both directions; the library's pbft_wire_decode_preprepare must give the same heads.  The replica tests are
the differential of tests/test_replica_streams.py -- the defining host sequence against pbft_replica_push_streams with
its front half on the host -- over PrePrepare traffic, with the heads switched on and off."""
import ctypes
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import pp_traffic as P
import streams_traffic as T
from conftest import ROOT
from replica_sim import DIGEST_FN, VERIFY_FN
from test_replica_streams import Pair

NATIVE = os.path.join(ROOT, "tests", "native")
BIN = os.path.join(NATIVE, "pp_main")
SRCS = [os.path.join(NATIVE, "pp_main.cpp")]
CSRC = os.path.join(ROOT, "pbft_amd", "csrc")
DEPS = SRCS + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + \
       [os.path.join(ROOT, "include", f) for f in os.listdir(os.path.join(ROOT, "include"))]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
SEQS = [1, 2, 3, 4, 5, 6]


def _build():
    if os.path.exists(BIN) and all(os.path.getmtime(d) <= os.path.getmtime(BIN) for d in DEPS):
        return
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    cmd = [HIPCC, "--offload-host-only", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer"] + SAN + \
          ["-o", BIN] + SRCS
    subprocess.run(cmd, check=True, timeout=600)


def native_heads(bodies, tmp_path):
    """Every body through the sanitized program, each in a heap buffer of exactly its length."""
    from pbft_amd.wire import PpHead
    _build()
    src, dst = str(tmp_path / "frames.bin"), str(tmp_path / "heads.bin")
    with open(src, "wb") as f:
        f.write(np.uint32(len(bodies)).tobytes())
        for b in bodies:
            f.write(np.uint32(len(b)).tobytes())
            f.write(b)
    env = dict(os.environ)
    sym = "/opt/rocm/lib/llvm/bin/llvm-symbolizer"
    if os.path.exists(sym):
        env["ASAN_SYMBOLIZER_PATH"] = sym
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0:halt_on_error=1"
    p = subprocess.run([BIN, src, dst], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    m = re.search(r"pp host run ok: (\d+) frames", p.stdout)
    assert m and int(m.group(1)) == len(bodies)
    return np.fromfile(dst, PpHead)


@pytest.fixture(scope="module")
def corpus():
    return P.corpus()


def parsed(body):
    from pbft_amd import PbftError, wire
    try:
        return wire.decode_json(body)
    except PbftError:
        return None


def check_ok_head(h, body):
    """PBFT_PP_OK implies: the general parser accepts the frame as a signed PrePrepare with these fields."""
    m = parsed(body)
    assert m is not None and m.kind == 0 and m.digest_ok and m.sig is not None, body
    op = body[int(h["op_off"]):int(h["op_off"]) + int(h["op_len"])]
    assert (m.view, m.seq, m.timestamp, m.replica) == (int(h["view"]), int(h["seq"]), int(h["timestamp"]),
                                                       int(h["replica"])), body
    assert m.digest == h["claimed"].tobytes() and m.sig == h["sig"].tobytes() and m.operation == op, body
    assert h["computed"].tobytes() == hashlib.blake2b(op, digest_size=64).digest(), body
    assert 1 <= len(m.client) <= 63 and P.in_alphabet(m.client.encode()) and P.in_alphabet(op) and len(op) <= P.OP_MAX


def test_differential_against_the_general_parser(corpus, tmp_path):
    from pbft_amd import wire
    bodies = [b for b, _ in corpus]
    heads = native_heads(bodies, tmp_path)
    assert len(heads) == len(bodies) > 10000
    n_ok = 0
    for h, (body, inside) in zip(heads, corpus):
        if h["status"] == wire.PP_OK:
            n_ok += 1
            check_ok_head(h, body)
        else:
            assert h["status"] == wire.PP_NONE and h.tobytes() == bytes(232), body
            assert not inside, body  # the allowed share of deferrals inside the form is zero
    assert n_ok > 30
    # the inputs called `inside` are what they claim, by the reference parser alone
    inside = [b for b, i in corpus if i]
    assert len(inside) >= 30
    for body in inside:
        m = parsed(body)
        assert m is not None and m.kind == 0 and m.sig is not None and P.in_alphabet(m.operation) and \
            len(m.operation) <= P.OP_MAX and 1 <= len(m.client) <= 63, body
    # no vote, ClientRequest, unsigned or non-ASCII frame is ever PBFT_PP_OK
    for h, (body, _) in zip(heads, corpus):
        if not body.startswith(b'{"PrePrepare":') or b'"signature"' not in body:
            assert h["status"] == wire.PP_NONE


def test_library_decoder_equals_the_sanitized_program(corpus, tmp_path):
    from pbft_amd import wire
    pick = [b for k, (b, i) in enumerate(corpus) if i or k % 7 == 0]
    heads = native_heads(pick, tmp_path)
    for h, body in zip(heads, pick):
        assert wire.decode_preprepare(body).tobytes() == h.tobytes(), body


def test_frame_length_window():
    from pbft_amd import wire
    hdr = open(os.path.join(ROOT, "include", "pbft_wire.h")).read()
    assert int(re.search(r"#define PBFT_PP_FRAME_MIN (\d+)\b", hdr).group(1)) == wire.PP_FRAME_MIN
    m = re.search(r"#define PBFT_PP_FRAME_MAX \((\d+) \+ PBFT_PP_OP_MAX\)", hdr)
    assert int(m.group(1)) + int(re.search(r"#define PBFT_PP_OP_MAX (\d+)\b", hdr).group(1)) == wire.PP_FRAME_MAX
    lo, hi, over = P.extremes()
    assert len(lo) == wire.PP_FRAME_MIN and len(hi) == wire.PP_FRAME_MAX and len(over) == wire.PP_FRAME_MAX + 1
    for body in (lo, hi):
        h = wire.decode_preprepare(body)
        assert h["status"] == wire.PP_OK
        check_ok_head(h, body)
    assert wire.decode_preprepare(over)["status"] == wire.PP_NONE
    assert wire.decode_preprepare(lo[:-1])["status"] == wire.PP_NONE
    assert wire.decode_preprepare(b"")["status"] == wire.PP_NONE


def test_symbols_and_arguments():
    import pbft_amd
    from pbft_amd import wire
    lib = pbft_amd.load()
    for f in ("pbft_wire_decode_preprepare", "pbft_wire_decode_preprepares_device", "pbft_verify_streams_admit_pp",
              "pbft_replica_set_streams_pp", "pbft_replica_get_pp_stats"):
        assert hasattr(lib, f), f
    for f in ("pbft_wire_decode_preprepare", "pbft_wire_decode_preprepares_device", "pbft_verify_streams_admit_pp"):
        assert f in pbft_amd.EXPORTS
    assert wire.PpHead.itemsize == 232
    assert [wire.PpHead.fields[k][1] for k in ("op_off", "replica", "status", "claimed", "computed", "sig")] == \
        [24, 32, 34, 40, 104, 168]
    out = np.zeros(1, wire.PpHead)
    assert lib.pbft_wire_decode_preprepare(None, 5, out.ctypes.data) == -1
    assert lib.pbft_wire_decode_preprepare(b"x", 1, None) == -1
    assert lib.pbft_wire_decode_preprepares_device(None, None, 0, None, None, 0, None, None) == -1
    n = None
    assert lib.pbft_verify_streams_admit_pp(n, n, 0, n, n, n, 0, 4, 8, 8, 8, 1, 0, 8, n, n, n, n, n, n, n, n, n, n) == -1
    lib.pbft_replica_set_streams_pp.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.pbft_replica_get_pp_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert lib.pbft_replica_set_streams_pp(None, 1) == -1 and lib.pbft_replica_get_pp_stats(None, None) == -1


# ---- the replica ----
class PpStats(ctypes.Structure):
    _fields_ = [("from_head", ctypes.c_uint64), ("from_parser", ctypes.c_uint64)]


def pp_stats(p, r):
    p.L.pbft_replica_get_pp_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(PpStats)]
    s = PpStats()
    assert p.L.pbft_replica_get_pp_stats(r, ctypes.byref(s)) == 0
    return s.from_head, s.from_parser


def set_pp(p, on):
    p.L.pbft_replica_set_streams_pp.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert p.L.pbft_replica_set_streams_pp(p.B, on) == 0


def count_pp(calls):
    frames = [f for c in calls for s in c for f in s["frames"]]
    canon = sum(P.canonical(f) for f in frames)
    return canon, sum(f.get("raw") is None and f["kind"] == T.PREPREPARE for f in frames) - canon


NAMES = sorted(P.kinds(4, SEQS))


@pytest.mark.parametrize("on", [1, 0])
@pytest.mark.parametrize("n", [4, 7])
@pytest.mark.parametrize("name", NAMES)
def test_each_kind(name, n, on):
    p = Pair(n)
    try:
        set_pp(p, on)
        calls = P.kinds(n, SEQS)[name]
        p.run(calls, name)
        s = p.sstats()
        assert s["calls_host_front"] == len(calls) and not any(v for k, v in s.items() if k.startswith("fallback_"))
        canon, other = count_pp(calls)
        assert canon > 0
        assert pp_stats(p, p.B) == ((canon, other) if on else (0, canon + other))
        assert pp_stats(p, p.A) == (0, canon + other)
    finally:
        p.close()


def test_what_the_kinds_exercise():
    named = P.kinds(4, SEQS)
    for name in ("honest", "escaped operation", "between votes"):
        p = Pair(4)
        try:
            p.run(named[name], name)
            assert all(p.L.pbft_replica_committed_local(p.B, T.VIEW, q) == 1 for q in SEQS), name
        finally:
            p.close()
    for name, field in (("relayed", "rejected_signer"), ("non-primary replica", "rejected_signer"),
                        ("digest mismatch", "rejected_digest"), ("two for one seq", "rejected_digest"),
                        ("same twice", "duplicates"), ("stale view", "rejected_view"),
                        ("outside the window", "rejected_watermark")):
        p = Pair(4)
        try:
            p.run(named[name], name)
            assert p.stats(p.B)[field] > 0, (name, field)
        finally:
            p.close()


@pytest.mark.parametrize("n", [4, 7])
def test_all_kinds_together(n):
    p = Pair(n)
    try:
        calls = T.together(P.kinds(n, SEQS))
        p.run(calls, "together")
        canon, other = count_pp(calls)
        assert pp_stats(p, p.B) == (canon, other) and other > 0 and canon > 20
    finally:
        p.close()


def test_digest_fn_sees_each_operation_once():
    """The override is called once per PrePrepare that reaches the digest -- from the primary, on the primary's
    connection -- with exactly the operation's bytes, where they lie in the caller's stream."""
    p = Pair(4)
    try:
        seen = []

        def digest(user, op, op_len, out):
            data = ctypes.string_at(op, op_len) if op_len else b""
            seen.append(data)
            ctypes.memmove(out, hashlib.blake2b(data, digest_size=64).digest(), 64)
            return 0
        df = DIGEST_FN(digest)
        assert p.L.pbft_replica_set_digest_fn(p.B, df, None) == 0
        named = P.kinds(4, SEQS)
        calls = named["honest"] + named["long operation"] + named["relayed"] + named["non-primary replica"]
        prim = T.VIEW % 4
        want = [f["op"] for c in calls for s in c for f in s["frames"]
                if f["kind"] == T.PREPREPARE and f["replica"] == prim and s["peer"] == prim]
        p.run(calls, "digest_fn")
        assert seen == want and len(want) > 8
        assert pp_stats(p, p.B)[1] == 0
    finally:
        p.close()


@pytest.mark.parametrize("on", [1, 0])
def test_no_digest_override_and_no_context(on):
    """A replica with a verifier override but neither a digest override nor a GPU context: with the heads the round
    commits (the digest comes with the head); without them the PrePrepare's digest has nowhere to run."""
    p = Pair(4)
    try:
        r = ctypes.c_void_p()
        assert p.L.pbft_replica_create(None, 4, 0, p.c.keys, ctypes.byref(r)) == 0
        vf = VERIFY_FN(p.c._oracle_verify)
        assert p.L.pbft_replica_set_verifier(r, vf, None) == 0
        assert p.L.pbft_replica_set_log_window(r, T.WINDOW) == 0
        old, p.B = p.B, r
        p.reps.append(r)
        set_pp(p, on)
        calls = T.materialize(P.kinds(4, SEQS)["honest"], p.sign_batch)
        if on:
            for c in calls:
                p.streams(*c)
            assert all(p.L.pbft_replica_committed_local(r, T.VIEW, q) == 1 for q in SEQS)
            assert pp_stats(p, r) == (len(SEQS), 0)
        else:
            stream, off, length, peer = calls[0]
            from test_replica_streams import SegHead
            from replica_sim import Event
            heads = (SegHead * len(off))()
            a, b, ne, ev = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32(), (Event * 64)()
            assert p.L.pbft_replica_push_streams(r, stream.ctypes.data, len(stream), off.ctypes.data,
                                                 length.ctypes.data, peer.ctypes.data, len(off), heads,
                                                 ctypes.byref(a), ctypes.byref(b), ev, 64, ctypes.byref(ne)) == -5
        p.B = old
    finally:
        p.close()
