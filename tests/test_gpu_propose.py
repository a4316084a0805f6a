"""The primary's proposals on the GPU: pbft_sign_preprepares_frames(_device) byte for byte against hashlib's digests, the
C oracle's RFC 8032 signatures and pbft_wire_encode_preprepares (tests/propose_sim.py) -- the stream, frame_off, the
digests, the signatures and the status -- over poisoned outputs with guards in front of and behind every buffer; then
the emitted frames into a backup's pbft_replica_push_streams, one capture and replay, and a GPU primary's
pbft_replica_propose against a twin that proposes through the CPU override."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import egress_sim as E
import propose_sim as P
from conftest import ROOT
from test_gpu_egress import REPLICAS, VALS
from test_gpu_verify import gv  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
POISON, GUARD = 0xA5, 512
SEED = hashlib.sha512(b"propose-seed").digest()[:32]
VIEW, FIRST = 10**19 - 1, 2**32 - 60  # 19 digits; the sequence numbers cross 2^32 - 1 -> 2^32 inside 130 requests
assert VALS == P.VALS and REPLICAS == P.REPLICAS


@pytest.fixture(scope="module")
def orc():
    o = ctypes.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))
    o.oracle_public_key.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    return E.bind_oracle(o)


@pytest.fixture(scope="module")
def sv(gv, orc):  # noqa: F811
    """The module's verifier with SEED installed as replica 2."""
    pk = ctypes.create_string_buffer(32)
    orc.oracle_public_key(pk, SEED)
    assert gv.set_signing_seed(SEED, 2).tobytes() == pk.raw
    yield gv
    gv.set_signing_seed(None)


_ref = {}


def reference(orc, n, salt=0, replica=2, view=VIEW, first=FIRST):
    """dict: the requests and everything both forms must return for them (computed once per key, never changed)."""
    key = (n, salt, replica, view, first)
    if key not in _ref:
        ops, ts, cl = P.mixed_ops(n, salt)
        if n >= 64:  # the last operation ends on the last byte of ops_bytes, which is no multiple of 16
            ops[-1], cl[-1] = b"z" * 129, "127.0.0.1:8080"
            if sum(len(o) for o in ops) % 16 == 0:
                ops[-1] += b"z"
            assert sum(len(o) for o in ops) % 16 != 0 and P.canonical(ops[-1], cl[-1])
        req, stream, off, dig, sig, st = P.reference(orc, SEED, replica, view, first, ops, ts, cl)
        dev, dev_off = P.device_reference(stream, off, st)
        _ref[key] = dict(ops=ops, ts=ts, cl=cl, req=req, stream=stream, off=off, dig=dig, sig=sig, st=st, dev=dev,
                         dev_off=dev_off, view=view, first=first)
    return _ref[key]


def guarded(torch, dev, size, align=0):
    """A poisoned device buffer of `size` bytes at 16-byte offset `align`, GUARD poisoned bytes on either side."""
    t = torch.full((GUARD + align + size + GUARD,), POISON, dtype=torch.uint8, device=dev)
    assert t.data_ptr() % 16 == 0
    return t


def body(t, size, align=0):
    a = t.cpu().numpy()
    assert (a[:GUARD + align] == POISON).all(), "bytes in front of an output overwritten"
    assert (a[GUARD + align + size:] == POISON).all(), "bytes behind an output overwritten"
    return a[GUARD + align:GUARD + align + size]


def run_device(v, req, n, view=VIEW, first=FIRST, align=0, cap=0, ops_bytes=None):
    """One device call over poisoned outputs -> (out [cap], frame_off, digests, sigs, status), every guard checked."""
    import torch
    dev = torch.device("cuda", 0)
    data, ob, off, ln, ts, cl = req
    ob = ob if ops_bytes is None else ops_bytes
    ins = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy() if a.size else
                            np.zeros(16, np.uint8)).to(dev) for a in (data, off, ln, ts, cl)]
    d_out, d_off = guarded(torch, dev, cap, align), guarded(torch, dev, 8 * (n + 1))
    d_dig, d_sig, d_st = guarded(torch, dev, 64 * n), guarded(torch, dev, 64 * n), guarded(torch, dev, n)
    s = torch.cuda.Stream()
    p = [t.data_ptr() for t in ins]
    v.sign_preprepares_frames_device(p[0], ob, p[1], p[2], p[3], p[4], view, first, n, d_out.data_ptr() + GUARD + align,
                                     cap, d_off.data_ptr() + GUARD, d_dig.data_ptr() + GUARD, d_sig.data_ptr() + GUARD,
                                     d_st.data_ptr() + GUARD, stream=s.cuda_stream)
    s.synchronize()
    return (body(d_out, cap, align), body(d_off, 8 * (n + 1)).copy().view(np.uint64),
            body(d_dig, 64 * n).reshape(n, 64), body(d_sig, 64 * n).reshape(n, 64), body(d_st, n))


def check_exact(v, r, align=0, slack=64):
    n = len(r["st"])
    total = len(r["dev"])
    out, off, dig, sig, st = run_device(v, r["req"], n, view=r["view"], first=r["first"], align=align,
                                        cap=total + slack)
    assert (st == r["st"]).all(), np.nonzero(st != r["st"])[0][:8]
    assert (off == r["dev_off"]).all(), np.nonzero(off != r["dev_off"])[0][:8]
    assert (dig == r["dig"]).all(), np.nonzero((dig != r["dig"]).any(axis=1))[0][:8]
    assert (sig == r["sig"]).all(), np.nonzero((sig != r["sig"]).any(axis=1))[0][:8]
    bad = np.nonzero(out[:total] != r["dev"])[0]
    assert bad.size == 0, (bad[:8], int(np.searchsorted(r["dev_off"], bad[0], side="right")) - 1)
    assert (out[total:] == POISON).all(), "bytes behind frame_off[N] overwritten"


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 130])
def test_byte_exact(sv, orc, n):
    r = reference(orc, n)
    if n >= 63:
        assert 0 < int((r["st"] == 0).sum()) < n  # general requests among canonical ones
    if n == 130:
        lens = {len(o) for o, s in zip(r["ops"], r["st"]) if s == 0}
        assert lens >= {0, 1, 127, 128, 129, 3071, 3072} and int(r["req"][1]) % 16 != 0
    check_exact(sv, r, align=n % 16)


@pytest.mark.parametrize("align", range(16))
def test_every_alignment_of_the_output(sv, orc, align):
    check_exact(sv, reference(orc, 130), align=align)


@pytest.mark.parametrize("replica", [0, 65534])
def test_replica_index_and_number_widths(sv, orc, replica):
    sv.set_signing_seed(SEED, replica)
    try:
        check_exact(sv, reference(orc, 65, salt=replica % 7 + 1, replica=replica, view=VALS[replica % 10],
                              first=2**64 - 65), align=3)
    finally:
        sv.set_signing_seed(SEED, 2)


@pytest.mark.parametrize("width", [1, 4, 16])
def test_other_forms_of_the_copy(sv, orc, width):
    """PBFT_OPT_PROPOSE_WIDTH changes the stores, not the bytes."""
    sv.set_option(sv.OPT_PROPOSE_WIDTH, width)
    try:
        r = reference(orc, 130)
        for align in (0, 5, 15):
            check_exact(sv, r, align=align)
        cap = int(r["dev_off"][70]) + 100
        out, off, _, _, _ = run_device(sv, r["req"], 130, align=9, cap=cap)
        end = int(r["dev_off"][70])
        assert (off == r["dev_off"]).all() and (out[:end] == r["dev"][:end]).all() and (out[end:] == POISON).all()
    finally:
        sv.set_option(sv.OPT_PROPOSE_WIDTH, 0)


@pytest.mark.parametrize("cut", ["mid_frame_mid_wave", "frame_boundary", "wave_boundary", "first_frame", "zero"])
def test_short_output(sv, orc, cut):
    """out_cap inside the stream: the frames that fit are exact, nothing at or beyond out_cap is written (nor between
    the last whole frame and out_cap), and frame_off, digests, sigs and status are complete."""
    r = reference(orc, 130)
    fo = r["dev_off"]
    ok = np.nonzero(r["st"] == 0)[0]
    a, b = int(ok[ok > 70][0]), int(ok[ok > 70][1])  # two canonical requests of the second wave
    fit, cap = {"mid_frame_mid_wave": (a, int(fo[a]) + 100), "frame_boundary": (b, int(fo[b])),
                "wave_boundary": (64, int(fo[64])), "first_frame": (0, 300), "zero": (0, 0)}[cut]
    assert int(r["st"][0]) == 0 and int(fo[1]) > 300
    out, off, dig, sig, st = run_device(sv, r["req"], 130, align=7, cap=cap)
    end = int(fo[fit])
    assert (off == fo).all() and int(off[-1]) == len(r["dev"]) > cap
    assert (dig == r["dig"]).all() and (sig == r["sig"]).all() and (st == r["st"]).all()
    assert (out[:end] == r["dev"][:end]).all()
    assert (out[end:] == POISON).all(), "a frame written in part, or bytes at or beyond out_cap"


def test_operation_outside_ops_bytes(sv, orc):
    """Such a request is not read: zero digest and signature, status GENERAL, its neighbours unaffected."""
    r = reference(orc, 65, salt=2)
    data, ob, off, ln, ts, cl = r["req"]
    off2, ln2 = off.copy(), ln.copy()
    off2[3] = ob - 1           # ends one byte behind ops_bytes
    ln2[3] = 2
    off2[64] = 2**63           # far outside
    ln2[40] = 2**32 - 1        # longer than everything
    out, foff, dig, sig, st = run_device(sv, (data, ob, off2, ln2, ts, cl), 65, cap=len(r["dev"]) + 64)
    want_st, want_dig, want_sig = r["st"].copy(), r["dig"].copy(), r["sig"].copy()
    for i in (3, 40, 64):
        want_st[i], want_dig[i], want_sig[i] = 1, 0, 0
    assert (st == want_st).all() and (dig == want_dig).all() and (sig == want_sig).all()
    lens = np.diff(r["dev_off"].astype(np.int64))
    lens[[3, 40, 64]] = 0
    assert (foff == np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)).all()
    keep = [i for i in range(65) if want_st[i] == 0]
    want = np.concatenate([r["dev"][int(r["dev_off"][i]):int(r["dev_off"][i + 1])] for i in keep])
    assert (out[:len(want)] == want).all() and (out[len(want):] == POISON).all()
    from pbft_amd import PbftError
    with pytest.raises(PbftError) as e:  # the blocking form refuses it
        sv.sign_preprepares_frames(VIEW, FIRST, (data, ob, off2, ln2, ts, cl))
    assert e.value.code == -1


def test_signing_clone_and_arguments(sv, orc):
    from pbft_amd import PbftError
    r = reference(orc, 5, salt=9)
    c = sv.clone()  # a clone does not inherit the seed: proposing without one is PBFT_EINVAL
    try:
        with pytest.raises(PbftError) as e:
            c.sign_preprepares_frames(VIEW, FIRST, r["req"])
        assert e.value.code == -1
        with pytest.raises(PbftError) as e:
            run_device(c, r["req"], 5, cap=1 << 16)
        assert e.value.code == -1
        c.set_signing_seed(SEED, 2)
        got = c.sign_preprepares_frames(VIEW, FIRST, r["req"])
        assert (got[0] == r["stream"]).all()
    finally:
        c.close()
    with pytest.raises(PbftError):  # first_seq + N - 1 wraps
        sv.sign_preprepares_frames(VIEW, 2**64 - 4, r["req"])
    with pytest.raises(PbftError):
        run_device(sv, r["req"], 5, first=2**64 - 4, cap=1 << 16)
    with pytest.raises(PbftError):
        sv.propose_reserve(2**24 + 1)


@pytest.mark.parametrize("n,salt", [(130, 0), (65, 4), (7, 5), (0, 0)])
def test_blocking_form(sv, orc, n, salt):
    """Equal to encode_preprepares on the mixed input: the general requests' frames are made on the host from the
    device's digests and signatures."""
    r = reference(orc, n, salt)
    stream, off, dig, sig, st = sv.sign_preprepares_frames(VIEW, FIRST, r["req"])
    assert (st == r["st"]).all() and (off == r["off"]).all() and (dig == r["dig"]).all() and (sig == r["sig"]).all()
    assert len(stream) == len(r["stream"]) and (stream == r["stream"]).all()


def test_blocking_form_all_canonical(sv, orc):
    ops = [b"testOperation"] * 70
    req, stream, off, dig, sig, st = P.reference(orc, SEED, 2, 1, 1, ops, list(range(70)), ["127.0.0.1:8080"] * 70)
    got = sv.sign_preprepares_frames(1, 1, req)
    assert (st == 0).all() and (got[0] == stream).all() and (got[1] == off).all() and (got[3] == sig).all()


def test_capture_and_replay(sv, orc):
    import torch
    n, dev = 130, torch.device("cuda", 0)
    refs = [reference(orc, n, salt=s) for s in (0, 11, 12)]
    cap = max(len(r["dev"]) for r in refs) + 64
    size = [max(a[k].nbytes for a in (r["req"] for r in refs)) for k in (0, 2, 3, 4, 5)]
    ob = max(r["req"][1] for r in refs)
    sv.propose_reserve(n)
    d_in = [torch.zeros(s + 16, dtype=torch.uint8, device=dev) for s in size]
    d_out = torch.full((cap + GUARD,), POISON, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_dig, d_sig = (torch.zeros(64 * n, dtype=torch.uint8, device=dev) for _ in range(2))
    d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
    p = [t.data_ptr() for t in d_in]
    args = (p[0], ob, p[1], p[2], p[3], p[4], VIEW, FIRST, n, d_out.data_ptr() + 1, cap, d_off.data_ptr(),
            d_dig.data_ptr(), d_sig.data_ptr(), d_st.data_ptr())

    def load(r):
        data, _, off, ln, ts, cl = r["req"]
        for t, a in zip(d_in, (data, off, ln, ts, cl)):
            b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
            t[:len(b)].copy_(torch.from_numpy(b.copy()))

    load(refs[0])
    sv.sign_preprepares_frames_device(*args)  # (an eager call first: the kernels are loaded)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sv.sign_preprepares_frames_device(*args, stream=torch.cuda.current_stream().cuda_stream)
    for r in refs[1:] + refs[:1]:
        load(r)
        d_out.fill_(POISON)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()[1:]
        assert (d_off.cpu().numpy().view(np.uint64) == r["dev_off"]).all()
        assert (d_dig.cpu().numpy().reshape(n, 64) == r["dig"]).all()
        assert (d_sig.cpu().numpy().reshape(n, 64) == r["sig"]).all()
        assert (d_st.cpu().numpy() == r["st"]).all()
        assert (out[:len(r["dev"])] == r["dev"]).all() and (out[len(r["dev"]):] == POISON).all()


def _gpu_replicas(c, L, count, me):
    from pbft_amd import GpuBatchVerifier
    gvs, reps = [], []
    for _ in range(count):
        g = GpuBatchVerifier(0)
        assert g.set_keys(c.keys_np.reshape(4, 32)).all()
        r = ctypes.c_void_p()
        assert L.pbft_replica_create(g._ctx, 4, me, c.keys, ctypes.byref(r)) == 0
        gvs.append(g)
        reps.append(r)
    return gvs, reps


def _push(L, rep, segs):
    """{peer: bytes} through pbft_replica_push_streams -> events."""
    from replica_sim import Event
    from test_replica_streams import SegHead
    order = sorted(segs)
    stream = np.frombuffer(b"".join(segs[s] for s in order) + bytes(16), np.uint8).copy()
    length = np.array([len(segs[s]) for s in order], np.uint64)
    off = (np.cumsum(length) - length).astype(np.uint64)
    peer = np.array(order, np.uint16)
    heads = (SegHead * max(1, len(order)))()
    a, b, ne, ev = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32(), (Event * 256)()
    assert L.pbft_replica_push_streams(rep, stream.ctypes.data, int(length.sum()), off.ctypes.data, length.ctypes.data,
                                       peer.ctypes.data, len(order), heads, ctypes.byref(a), ctypes.byref(b), ev, 256,
                                       ctypes.byref(ne)) == 0
    return [(e.view, e.seq, e.kind) for e in ev[:ne.value]]


def test_round_trip_into_a_backups_streams_path(orc):
    """16 canonical requests framed by the primary's context, sent from the primary's connection into a GPU backup's
    pbft_replica_push_streams: every PrePrepare is taken from its device-made head."""
    from replica_sim import EV_PRE_PREPARED, Cluster
    from test_pp import pp_stats
    from test_replica_streams import bind as bind_streams
    c = Cluster(4, use_oracle_verifier=False)
    L = bind_streams(P.bind(E.bind(c.L)))
    view, p = 1, c.primary(1)
    gvs, reps = _gpu_replicas(c, L, 1, me=2)
    try:
        g = gvs[0].clone()
        try:
            g.set_signing_seed(c.seeds[p], p)
            ops = [b"request-%d" % i * (1 + 7 * i) for i in range(16)]
            frames = g.sign_preprepares_frames(view, 1, wire_requests(ops))
        finally:
            g.close()
        assert (frames[4] == 0).all()
        ev = _push(L, reps[0], {p: frames[0].tobytes()})
        assert ev == [(view, q, EV_PRE_PREPARED) for q in range(1, 17)]
        assert pp_stats(c, reps[0]) == (16, 0)
    finally:
        for r in reps:
            L.pbft_replica_destroy(r)
        for g in gvs:
            g.close()
        c.close()


def wire_requests(ops):
    from pbft_amd import wire
    return wire.pack_requests(ops, list(range(1, len(ops) + 1)), ["127.0.0.1:8080"] * len(ops))


def test_gpu_primary_against_the_cpu_twin(orc):
    """n = 4, the primary of view 1: the replica that hashes, signs and frames on the GPU proposes the bytes its twin
    proposes through the oracle override; with the loopback both report the same events after the flush, and their own
    Prepares are identical."""
    from replica_sim import EV_PRE_PREPARED, Cluster
    from test_replica_streams import bind as bind_streams
    c = Cluster(4, use_oracle_verifier=False)
    L = bind_streams(P.bind(E.bind(c.L)))
    view, me = 1, c.primary(1)
    gvs, reps = _gpu_replicas(c, L, 2, me)
    try:
        gpu, twin = reps
        ops, ts, cl = P.mixed_ops(40, salt=6)
        from pbft_amd import wire
        req = wire.pack_requests(ops, ts, cl)
        assert P.propose(L, gpu, req, cap=1 << 20)[0] == P.EINVAL  # no signer yet
        assert L.pbft_replica_set_signing_seed(gpu, c.seeds[me]) == 0
        proposer = P.OracleProposer(c.o, c.seeds[me])
        proposer.install(L, twin)
        signer = E.OracleSigner(orc, c.seeds[me])  # (the twin's outbox: its own Prepares)
        signer.install(L, twin)
        outs = [P.propose(L, r, req, flags=P.PROPOSE_LOOPBACK) for r in (gpu, twin)]
        assert outs[0][0] == outs[1][0] == 0 and outs[0][2:] == outs[1][2:] and outs[0][4] == 40
        assert outs[0][1].tobytes() == outs[1][1].tobytes()
        assert proposer.calls == 1
        events = [_push(L, r, {}) for r in (gpu, twin)]  # the flush: their own PrePrepares verified like anyone's
        assert events[0] == events[1] == [(view, q, EV_PRE_PREPARED) for q in range(1, 41)]
        st = [P.propose_stats(L, r) for r in (gpu, twin)]
        assert all((s["proposed"], s["calls"], s["held_back"], s["loopback_applied"]) == (40, 1, 0, 40) for s in st)
        emitted = [E.emit(L, r) for r in (gpu, twin)]
        assert emitted[0][0] == emitted[1][0] == 0 and emitted[0][3] == emitted[1][3] == 40
        assert emitted[0][1].tobytes() == emitted[1][1].tobytes()
    finally:
        for r in reps:
            L.pbft_replica_destroy(r)
        for g in gvs:
            g.close()
        c.close()
