"""The primary's proposals without a GPU: pbft_wire_encode_preprepares against pbft_wire_encode_frame message by message
and against the ingress matcher (pbft_wire_decode_preprepare) in both directions; pbft_replica_propose under a proposer
override (hashlib digests, the C oracle's signatures; tests/propose_sim.py) against a twin fed the same PrePrepares by
hand; and the frame rule with the host encoder as a stand-alone program under AddressSanitizer + UBSan
(tests/native/propose_main.cpp)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import egress_sim as E
import propose_sim as P
from conftest import ROOT
from pbft_amd import wire
from replica_sim import EV_PRE_PREPARED, Cluster

VIEW = 1


# ---- the encoder ----
def check_encoder(view, first_seq, replica, n, salt):
    ops, ts, cl = P.mixed_ops(n, salt)
    req = wire.pack_requests(ops, ts, cl)
    rng = np.random.default_rng(salt)
    dig, sig = rng.integers(0, 256, (n, 64), dtype=np.uint8), rng.integers(0, 256, (n, 64), dtype=np.uint8)
    stream, off, st = wire.encode_preprepares(view, first_seq, req, replica, dig, sig)
    assert int(off[0]) == 0 and int(off[-1]) == len(stream)
    n_ok = 0
    for i in range(n):
        frame = stream[int(off[i]):int(off[i + 1])].tobytes()
        want = wire.encode_frame(wire.WireMsg(kind=wire.PREPREPARE, view=view, seq=first_seq + i, digest=dig[i].tobytes(),
                                              replica=replica, sig=sig[i].tobytes(), operation=ops[i], timestamp=ts[i],
                                              client=cl[i]))
        assert frame == want, (i, ops[i][:8], cl[i])
        assert int(st[i]) == (wire.PROPOSE_OK if P.canonical(ops[i], cl[i]) else wire.PROPOSE_GENERAL), i
        body_len, hn = wire.uvi_decode(frame[:10])
        body = frame[hn:]
        assert len(body) == body_len
        h = wire.decode_preprepare(body)
        assert (int(h["status"]) == wire.PP_OK) == (int(st[i]) == wire.PROPOSE_OK), i  # both directions
        if int(st[i]) == wire.PROPOSE_OK:
            n_ok += 1
            assert hn == 2 and wire.PP_FRAME_MIN <= body_len <= wire.PP_FRAME_MAX
            assert (int(h["view"]), int(h["seq"]), int(h["timestamp"]), int(h["replica"])) == \
                (view, first_seq + i, ts[i], replica)
            assert body[int(h["op_off"]):int(h["op_off"]) + int(h["op_len"])] == ops[i]
            assert h["claimed"].tobytes() == dig[i].tobytes() and h["sig"].tobytes() == sig[i].tobytes()
            assert h["computed"].tobytes() == P.digests_of([ops[i]])[0].tobytes()
    return n_ok, st


def test_symbols_exported():
    import pbft_amd
    lib = pbft_amd.load()
    for f in ("pbft_wire_encode_preprepares", "pbft_propose_reserve", "pbft_sign_preprepares_frames_device",
              "pbft_sign_preprepares_frames"):
        assert hasattr(lib, f) and f in pbft_amd.EXPORTS
    for f in ("pbft_replica_propose", "pbft_replica_set_next_seq", "pbft_replica_set_proposer",
              "pbft_replica_get_propose_stats"):
        assert hasattr(lib, f)


def test_mix_covers_the_cases():
    ops, ts, cl = P.mixed_ops(130)
    can = [P.canonical(o, c) for o, c in zip(ops, cl)]
    assert {len(o) for o in ops} == set(P.OP_LENS)
    assert {len(o) for o, k in zip(ops, can) if k} == set(P.OP_LENS) - {3073}  # every canonical length, 0 and 3072 too
    assert {len(c) for c in cl} >= {0, 1, 63, 64} and {len(c) for c, k in zip(cl, can) if k} >= {1, 63}
    for sp in P.SPECIALS:
        assert any(o.startswith(sp) for o in ops) and any(o.endswith(sp) and len(o) > len(sp) for o in ops), sp
    assert 30 < sum(can) < 100


@pytest.mark.parametrize("k", range(10))
def test_encoder_against_encode_frame(k):
    """View, first_seq and the timestamps walk the decimal-width edges (first_seq so that the width changes inside the
    batch where it can); the replica index walks its own."""
    view = P.VALS[k]
    first_seq = [0, 7, 97, 2**32 - 3, 10**19 - 5, 2**64 - 40, 1, 9, 99, 10**19 - 1][k]
    n_ok, st = check_encoder(view, first_seq, P.REPLICAS[k % 8], 40, salt=k)
    assert 0 < n_ok < 40


def test_encoder_every_case_of_the_mix():
    n_ok, st = check_encoder(1, 1, 2, 130, salt=0)
    assert n_ok == int((st == 0).sum()) > 30


def test_length_query_short_cap_and_wrap():
    lib = wire.load()
    ops, ts, cl = P.mixed_ops(24, salt=3)
    req = wire.pack_requests(ops, ts, cl)
    data, _, off, ln, t, c = req
    dig = sig = np.zeros((24, 64), np.uint8)
    stream, foff, st = wire.encode_preprepares(3, 5, req, 1, dig, sig)
    need = ctypes.c_size_t()
    args = (24, 3, 5, data.ctypes.data, off.ctypes.data, ln.ctypes.data, t.ctypes.data, c.ctypes.data, 1)
    # the length query needs neither digests nor signatures, and fills frame_off and status
    f2, s2 = np.zeros(25, np.uint64), np.zeros(24, np.uint8)
    assert lib.pbft_wire_encode_preprepares(*args, None, None, None, 0, ctypes.byref(need), f2.ctypes.data,
                                            s2.ctypes.data) == 0
    assert need.value == len(stream) and (f2 == foff).all() and (s2 == st).all()
    # a short cap: PBFT_EINVAL, the length still reported, nothing behind cap touched
    for cap in (len(stream) - 1, int(foff[7]) + 5, 1):
        out = np.full(len(stream) + 64, 0xA5, np.uint8)
        need.value = 0
        assert lib.pbft_wire_encode_preprepares(*args, dig.ctypes.data, sig.ctypes.data, out.ctypes.data, cap,
                                                ctypes.byref(need), None, None) == P.EINVAL
        assert need.value == len(stream) and (out[cap:] == 0xA5).all()
    # without digests a real encode is refused
    out = np.zeros(len(stream), np.uint8)
    assert lib.pbft_wire_encode_preprepares(*args, None, None, out.ctypes.data, len(stream), ctypes.byref(need), None,
                                            None) == P.EINVAL
    # first_seq + i wraps
    wrap = (24, 3, 2**64 - 23) + args[3:]
    assert lib.pbft_wire_encode_preprepares(*wrap, None, None, None, 0, ctypes.byref(need), None, None) == P.EINVAL
    last = (24, 3, 2**64 - 24) + args[3:]
    assert lib.pbft_wire_encode_preprepares(*last, None, None, None, 0, ctypes.byref(need), None, None) == 0
    assert lib.pbft_wire_encode_preprepares(*(args[:8] + (65536,)), None, None, None, 0, ctypes.byref(need), None,
                                            None) == P.EINVAL
    assert lib.pbft_wire_encode_preprepares(0, 1, 2**64 - 1, None, None, None, None, None, 0, None, None, None, 0,
                                            ctypes.byref(need), f2.ctypes.data, None) == 0
    assert need.value == 0 and int(f2[0]) == 0


# ---- the replica ----
class Net(Cluster):
    """A 4-replica cluster (view 1: replica 1 is the primary) whose replicas propose through the oracle override."""

    def __init__(self, proposers=(1,), signers=()):
        super().__init__(4)
        P.bind(E.bind(self.L))
        self.proposers, self.signers = {}, {}
        for i in proposers:
            self.proposers[i] = P.OracleProposer(self.o, self.seeds[i])
            self.proposers[i].install(self.L, self.reps[i])
        for i in signers:
            self.signers[i] = E.OracleSigner(self.o, self.seeds[i])
            self.signers[i].install(self.L, self.reps[i])


CANON = ([b"testOperation", b"", b"x" * 3072, b"second operation", b"y" * 129], [1, 2, 3, 10**19, 5],
         ["127.0.0.1:8080", "c", P.C63, "127.0.0.1:8080", "[::1]:9"])


def test_replica_bytes_and_twin():
    """The primary's bytes are encode_preprepares of hand-made digests and signatures (general requests among them),
    and with the loopback it stands where a twin stands that was handed the same PrePrepares one by one."""
    a, b = Net(signers=[1]), Net(proposers=(), signers=[1])
    try:
        p = a.primary(VIEW)
        ops, ts, cl = P.mixed_ops(24, salt=1)
        req, stream, off, dig, sig, st = P.reference(a.o, a.seeds[p], p, VIEW, 1, ops, ts, cl)
        assert 0 < int((st == 0).sum()) < 24
        rc, out, n, first, n_prop = P.propose(a.L, a.reps[p], req, flags=P.PROPOSE_LOOPBACK)
        assert (rc, n, first, n_prop) == (0, len(stream), 1, 24) and out.tobytes() == stream.tobytes()
        assert a.proposers[p].calls == 1
        for i in range(24):
            assert b.L.pbft_replica_on_pre_prepare(b.reps[p], p, VIEW, 1 + i, ops[i], len(ops[i]), dig[i].tobytes(),
                                                   sig[i].tobytes(), None) == 1
        ev = [c.flush(p, force=1) for c in (a, b)]
        assert ev[0] == ev[1] == [(VIEW, 1 + i, EV_PRE_PREPARED) for i in range(24)]
        sa, sb = a.stats(p), b.stats(p)
        assert all(sa[k] == sb[k] for k in sa if not k.endswith("_ns")), (sa, sb)
        assert sa["accepted"] == 24 and sa["rejected_sig"] == 0  # the primary's own PrePrepares verified like anyone's
        outs = [E.emit(c.L, c.reps[p]) for c in (a, b)]  # the outbox: its own Prepares
        assert outs[0][3] == outs[1][3] == 24 and outs[0][1].tobytes() == outs[1][1].tobytes()
        ps = P.propose_stats(a.L, a.reps[p])
        assert (ps["proposed"], ps["calls"], ps["held_back"], ps["loopback_applied"]) == (24, 1, 0, 24)
    finally:
        a.close()
        b.close()


def test_without_loopback_nothing_is_applied():
    c = Net()
    try:
        p = c.primary(VIEW)
        req = wire.pack_requests(*CANON)
        rc, out, n, first, n_prop = P.propose(c.L, c.reps[p], req)
        assert (rc, first, n_prop) == (0, 1, 5)
        assert c.flush(p, force=1) == [] and c.stats(p)["pushed"] == 0
        assert P.propose_stats(c.L, c.reps[p])["loopback_applied"] == 0
    finally:
        c.close()


def test_a_backup_refuses_and_no_signer_is_an_error():
    c = Net(proposers=(0, 1, 2, 3))
    try:
        req = wire.pack_requests(*CANON)
        for i in (0, 2, 3):
            rc, out, n, first, n_prop = P.propose(c.L, c.reps[i], req, cap=1 << 16)
            assert (rc, n, n_prop) == (P.EINVAL, 0, 0) and c.proposers[i].calls == 0
            assert P.propose_stats(c.L, c.reps[i]) == dict(proposed=0, calls=0, held_back=0, loopback_applied=0,
                                                           propose_ns=0)
        p = c.primary(VIEW)
        assert c.L.pbft_replica_set_proposer(c.reps[p], P.PROPOSER_FN(), None) == 0  # removed: no seed either
        need, first, n_prop = ctypes.c_size_t(), ctypes.c_uint64(), ctypes.c_uint64()
        data, ob, off, ln, ts, cl = req
        args = (c.reps[p], 5, data.ctypes.data, ob, off.ctypes.data, ln.ctypes.data, ts.ctypes.data, cl.ctypes.data)
        assert c.L.pbft_replica_propose(*args, 0, None, 0, ctypes.byref(need), ctypes.byref(first),
                                        ctypes.byref(n_prop)) == 0  # (the size query needs no signer)
        buf = np.zeros(need.value, np.uint8)
        assert c.L.pbft_replica_propose(*args, 0, buf.ctypes.data, need.value, ctypes.byref(need), ctypes.byref(first),
                                        ctypes.byref(n_prop)) == P.EINVAL
        c.proposers[p].install(c.L, c.reps[p])
        assert P.propose(c.L, c.reps[p], req)[3:] == (1, 5)  # ... and no sequence number was consumed
        # an operation outside ops_bytes, an unknown flag
        bad = (data, ob - 1, off, ln, ts, cl)
        assert P.propose(c.L, c.reps[p], bad, cap=1 << 16)[0] == P.EINVAL
        assert P.propose(c.L, c.reps[p], req, flags=2, cap=1 << 16)[0] == P.EINVAL
        assert P.propose(c.L, c.reps[p], req)[3:] == (6, 5)
    finally:
        c.close()


def test_window_holds_requests_back():
    c = Net()
    try:
        p = c.primary(VIEW)
        assert c.L.pbft_replica_set_log_window(c.reps[p], 8) == 0
        ops = [b"op-%d" % i for i in range(11)]
        req = wire.pack_requests(ops, list(range(11)), ["127.0.0.1:8080"] * 11)
        _, stream, off, dig, sig, st = P.reference(c.o, c.seeds[p], p, VIEW, 1, ops, list(range(11)),
                                                   ["127.0.0.1:8080"] * 11)
        rc, out, n, first, n_prop = P.propose(c.L, c.reps[p], req, flags=P.PROPOSE_LOOPBACK)
        assert (rc, first, n_prop) == (0, 1, 8) and out.tobytes() == stream[:int(off[8])].tobytes()
        assert P.propose_stats(c.L, c.reps[p])["held_back"] == 3
        rest = P.slice_requests(req, 8, 11)
        rc, out, n, first, n_prop = P.propose(c.L, c.reps[p], rest, flags=P.PROPOSE_LOOPBACK, cap=64)
        assert (rc, n, first, n_prop) == (0, 0, 9, 0)  # the window is full
        assert P.propose_stats(c.L, c.reps[p])["held_back"] == 6
        assert len(c.flush(p, force=1)) == 8
        assert c.L.pbft_replica_stable_checkpoint(c.reps[p], 4) == 0
        rc, out, n, first, n_prop = P.propose(c.L, c.reps[p], rest, flags=P.PROPOSE_LOOPBACK)
        assert (rc, first, n_prop) == (0, 9, 3) and out.tobytes() == stream[int(off[8]):].tobytes()
        assert c.flush(p, force=1) == [(VIEW, q, EV_PRE_PREPARED) for q in (9, 10, 11)]
        ps = P.propose_stats(c.L, c.reps[p])
        assert (ps["proposed"], ps["calls"], ps["held_back"], ps["loopback_applied"]) == (11, 2, 6, 11)
    finally:
        c.close()


def test_set_next_seq_and_the_low_watermark():
    c = Net()
    try:
        p = c.primary(VIEW)
        req = wire.pack_requests(*CANON)
        assert c.L.pbft_replica_set_next_seq(c.reps[p], 100) == 0
        rc, out, n, first, n_prop = P.propose(c.L, c.reps[p], req)
        _, stream, _, _, _, _ = P.reference(c.o, c.seeds[p], p, VIEW, 100, *CANON)
        assert (rc, first, n_prop) == (0, 100, 5) and out.tobytes() == stream.tobytes()
        assert P.propose(c.L, c.reps[p], req)[3:] == (105, 5)
        assert c.L.pbft_replica_stable_checkpoint(c.reps[p], 500) == 0  # seqs start at max(next_seq, h + 1)
        assert P.propose(c.L, c.reps[p], req)[3:] == (501, 5)
        assert c.L.pbft_replica_set_next_seq(c.reps[p], 7) == 0
        assert P.propose(c.L, c.reps[p], req)[3:] == (501, 5)
    finally:
        c.close()


def test_short_cap_consumes_no_seq():
    c = Net()
    try:
        p = c.primary(VIEW)
        req = wire.pack_requests(*CANON)
        _, stream, _, _, _, _ = P.reference(c.o, c.seeds[p], p, VIEW, 1, *CANON)
        rc, out, n, first, n_prop = P.propose(c.L, c.reps[p], req, flags=P.PROPOSE_LOOPBACK, cap=len(stream) - 1)
        assert (rc, n, first, n_prop) == (P.EINVAL, len(stream), 1, 5) and c.proposers[p].calls == 0
        assert c.stats(p)["pushed"] == 0 and P.propose_stats(c.L, c.reps[p])["calls"] == 0
        rc, out, n, first, n_prop = P.propose(c.L, c.reps[p], req, cap=len(stream))
        assert (rc, n, first, n_prop) == (0, len(stream), 1, 5) and out.tobytes() == stream.tobytes()
    finally:
        c.close()


def test_a_backup_ingests_the_emitted_bytes():
    c = Net()
    try:
        p = c.primary(VIEW)
        ops = [b"request %d" % i for i in range(6)] + [b'an "escaped" one']
        ts, cl = list(range(7)), ["127.0.0.1:8080"] * 7
        rc, out, n, first, n_prop = P.propose(c.L, c.reps[p], wire.pack_requests(ops, ts, cl))
        assert rc == 0 and n_prop == 7
        used, pushed, dropped = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        assert c.L.pbft_replica_push_frames(c.reps[2], p, out.tobytes(), len(out), ctypes.byref(used),
                                            ctypes.byref(pushed), ctypes.byref(dropped)) == 0
        assert (used.value, pushed.value, dropped.value) == (len(out), 7, 0)
        assert c.flush(2, force=1) == [(VIEW, q, EV_PRE_PREPARED) for q in range(1, 8)]
        # the same bytes from another replica's connection are not the primary's
        assert c.L.pbft_replica_push_frames(c.reps[3], 0, out.tobytes(), len(out), ctypes.byref(used),
                                            ctypes.byref(pushed), ctypes.byref(dropped)) == 0
        assert c.flush(3, force=1) == [] and c.stats(3)["rejected_signer"] == 7
    finally:
        c.close()


# ---- the stand-alone sanitizer run ----
NATIVE = os.path.join(ROOT, "tests", "native")
BIN = os.path.join(NATIVE, "propose_main")
SRCS = [os.path.join(NATIVE, "propose_main.cpp"), os.path.join(ROOT, "pbft_amd", "csrc", "host", "wire.cpp")]
CSRC = os.path.join(ROOT, "pbft_amd", "csrc")
DEPS = SRCS + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + \
       [os.path.join(ROOT, "include", f) for f in os.listdir(os.path.join(ROOT, "include"))]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]


def test_frame_rule_and_encoder_clean_under_asan_ubsan():
    if not (os.path.exists(BIN) and all(os.path.getmtime(d) <= os.path.getmtime(BIN) for d in DEPS)):
        if not os.path.exists(HIPCC):
            pytest.skip("hipcc not present")
        subprocess.run([HIPCC, "--offload-host-only", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer"] + SAN +
                       ["-o", BIN] + SRCS, check=True, timeout=600)
    env = dict(os.environ)
    sym = "/opt/rocm/lib/llvm/bin/llvm-symbolizer"
    if os.path.exists(sym):
        env["ASAN_SYMBOLIZER_PATH"] = sym
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0:halt_on_error=1"
    p = subprocess.run([BIN, "300"], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    m = re.search(r"propose host run ok: (\d+) frames, (\d+) canonical", p.stdout)
    assert m and int(m.group(1)) > 800 and 100 < int(m.group(2)) < int(m.group(1))
