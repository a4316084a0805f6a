"""Replica egress on the GPU: pbft_sign_set_seed / pbft_sign_votes_frames(_device) byte for byte against the C oracle's
RFC 8032 signatures encoded by pbft_wire_encode_votes (tests/egress_sim.py) -- the stream, frame_off and the
signatures -- then the emitted frames back through the ingress chain, one capture and replay, and a GPU replica's
pbft_replica_emit_frames against a twin that signs through the CPU override."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import egress_sim as E
from conftest import ROOT
from test_gpu_verify import gv, seeds_for  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
POISON, GUARD = 0xA5, 512
VALS = [0, 9, 10, 99, 100, 2**32 - 1, 2**32, 10**19 - 1, 10**19, 2**64 - 1]
REPLICAS = [0, 9, 10, 999, 1000, 9999, 10000, 65534]
SEED = hashlib.sha512(b"egress-seed").digest()[:32]


@pytest.fixture(scope="module")
def orc():
    o = ctypes.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))
    o.oracle_public_key.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    return E.bind_oracle(o)


def make_env(n, salt=0):
    """Both kinds in turn; view and seq walk VALS so that every pair of widths occurs within 200 envelopes: envelope 1
    is the shortest form (a Commit with one-digit numbers), envelope 56 the longest (a Prepare with 20-digit ones)."""
    rng = np.random.default_rng(1000 + salt)
    i = np.arange(n)
    j = i >> 1
    view = np.array([VALS[k % 10] for k in j], np.uint64)
    seq = np.array([VALS[(7 * k + k // 10) % 10] for k in j], np.uint64)
    return E.envelopes(1 + (i & 1), view, seq, rng.integers(0, 256, (n, 64), dtype=np.uint8))


_ref = {}


def reference(orc, n, replica, salt=0):
    key = (n, replica, salt)
    if key not in _ref:
        env = make_env(n, salt)
        _ref[key] = (env,) + E.oracle_frames(orc, SEED, replica, env)
    return _ref[key]


@pytest.fixture(scope="module")
def sv(gv, orc):  # noqa: F811
    """The module's verifier with SEED installed (replica 2 until a test says otherwise)."""
    pk = ctypes.create_string_buffer(32)
    orc.oracle_public_key(pk, SEED)
    assert gv.set_signing_seed(SEED, 2).tobytes() == pk.raw
    return gv


def run_device(v, env, stride=85, align=0, out_cap=None, total=None, graph=None):
    """One device call over poisoned outputs; -> (out buffer behind the alignment shift, frame_off, sigs).  The guards in
    front of d_out, behind frame_off and behind sigs are checked here; the bytes behind the stream by the caller."""
    import torch
    dev = torch.device("cuda", 0)
    n = len(env)
    rows = np.full(max((n - 1) * stride + 85, 1) if n else 1, 0xEE, np.uint8)
    for i in range(n):
        rows[i * stride:i * stride + 85] = env[i]
    d_env = torch.from_numpy(rows).to(dev)
    cap = out_cap if out_cap is not None else total
    d_out = torch.full((align + cap + GUARD,), POISON, dtype=torch.uint8, device=dev)
    d_off = torch.full((8 * (n + 1) + GUARD,), POISON, dtype=torch.uint8, device=dev)
    d_sig = torch.full((64 * n + GUARD,), POISON, dtype=torch.uint8, device=dev)
    assert d_out.data_ptr() % 16 == 0
    ts = torch.cuda.Stream()
    v.sign_votes_frames_device(d_env.data_ptr() if n else 0, n, d_out.data_ptr() + align, cap, d_off.data_ptr(),
                               d_sig.data_ptr(), env_stride=stride, stream=ts.cuda_stream)
    ts.synchronize()
    out, off, sig = d_out.cpu().numpy(), d_off.cpu().numpy(), d_sig.cpu().numpy()
    assert (out[:align] == POISON).all(), "bytes in front of d_out overwritten"
    assert (off[8 * (n + 1):] == POISON).all() and (sig[64 * n:] == POISON).all()
    return out[align:], off[:8 * (n + 1)].view(np.uint64).copy(), sig[:64 * n].reshape(n, 64).copy()


def check_exact(v, orc, n, replica=2, stride=85, align=0):
    env, stream, frame_off, sigs = reference(orc, n, replica)
    out, off, sig = run_device(v, env, stride, align, total=len(stream))
    assert (off == frame_off).all(), np.nonzero(off != frame_off)[0][:8]
    assert (sig == sigs).all(), np.nonzero((sig != sigs).any(axis=1))[0][:8]
    bad = np.nonzero(out[:len(stream)] != stream)[0]
    assert bad.size == 0, (bad[:8], int(np.searchsorted(frame_off, bad[0], side="right")) - 1)
    assert (out[len(stream):] == POISON).all(), "bytes behind frame_off[N] overwritten"
    return frame_off


def test_seed_and_its_public_key(sv, orc):
    from pbft_amd import PbftError
    c = sv.clone()  # a clone does not inherit the seed: signing without one is PBFT_EINVAL
    try:
        env = make_env(2)
        with pytest.raises(PbftError) as e:
            c.sign_votes_frames(env)
        assert e.value.code == -1
        with pytest.raises(PbftError) as e:
            run_device(c, env, total=800)
        assert e.value.code == -1
        pk = ctypes.create_string_buffer(32)
        for tag in range(3):
            seed = hashlib.sha256(b"seed-%d" % tag).digest()
            orc.oracle_public_key(pk, seed)
            assert c.set_signing_seed(seed, 7).tobytes() == pk.raw
        stream, off, sigs = c.sign_votes_frames(env)
        want = E.oracle_frames(orc, seed, 7, env)
        assert (stream == want[0]).all() and (off == want[1]).all() and (sigs == want[2]).all()
        c.set_signing_seed(None)
        with pytest.raises(PbftError):
            c.sign_votes_frames(env)
        with pytest.raises(PbftError):
            c.set_signing_seed(SEED, 65536)
    finally:
        c.close()


@pytest.mark.parametrize("stride", [85, 96])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 130, 193, 4133])
def test_byte_exact(sv, orc, n, stride):
    """N around the 64-envelope scan tile (130 and 193 span three and four tiles) and, at 4,133, two 64-tile steps of
    the scan over the tiles."""
    sv.set_signing_seed(SEED, 2)
    check_exact(sv, orc, n, stride=stride, align=n % 16)


@pytest.mark.parametrize("replica", REPLICAS)
def test_every_width_of_the_replica_index(sv, orc, replica):
    sv.set_signing_seed(SEED, replica)
    try:
        lens = np.diff(check_exact(sv, orc, 130, replica=replica, align=3))
        assert lens.min() == 338 + len(str(replica)) - 1 and lens.max() == 381 - 5 + len(str(replica))
        if replica < 10:
            assert lens.min() == 338  # the shortest frame there is
        if replica >= 10000:
            assert lens.max() == 381  # and the longest
    finally:
        sv.set_signing_seed(SEED, 2)


@pytest.mark.parametrize("align", range(16))
def test_every_alignment_of_the_output(sv, orc, align):
    sv.set_signing_seed(SEED, 2)
    check_exact(sv, orc, 130, align=align)


@pytest.mark.parametrize("block,direct", [(256, 0), (64, 1), (256, 1)])
def test_other_forms_of_the_signing_kernel(sv, orc, block, direct):
    """PBFT_OPT_EGRESS_BLOCK / _DIRECT change the launch, not the bytes."""
    sv.set_signing_seed(SEED, 2)
    sv.set_option(sv.OPT_EGRESS_BLOCK, block)
    sv.set_option(sv.OPT_EGRESS_DIRECT, direct)
    try:
        check_exact(sv, orc, 321, align=5)
        env, stream, frame_off, _ = reference(orc, 321, 2)
        cap = int(frame_off[200]) + 77
        out, off, _ = run_device(sv, env, align=5, out_cap=cap)
        assert (off == frame_off).all() and (out[:int(frame_off[200])] == stream[:int(frame_off[200])]).all()
        assert (out[int(frame_off[200]):] == POISON).all()
    finally:
        sv.set_option(sv.OPT_EGRESS_BLOCK, 0)
        sv.set_option(sv.OPT_EGRESS_DIRECT, 0)


@pytest.mark.parametrize("cut", ["mid_frame_mid_wave", "frame_boundary", "wave_boundary", "first_frame", "zero"])
def test_short_output(sv, orc, cut):
    """out_cap inside the stream: the frames that fit are exact, nothing at or beyond out_cap is written (nor between
    the last whole frame and out_cap), frame_off[N] is still the full length."""
    sv.set_signing_seed(SEED, 2)
    env, stream, frame_off, sigs = reference(orc, 130, 2)
    fit, cap = {"mid_frame_mid_wave": (70, int(frame_off[70]) + 100), "frame_boundary": (71, int(frame_off[71])),
                "wave_boundary": (64, int(frame_off[64])), "first_frame": (0, 337), "zero": (0, 0)}[cut]
    out, off, sig = run_device(sv, env, align=7, out_cap=cap)
    end = int(frame_off[fit])
    assert (off == frame_off).all() and int(off[-1]) == len(stream) > cap
    assert (sig == sigs).all()
    assert (out[:end] == stream[:end]).all()
    assert (out[end:] == POISON).all(), "a frame written in part, or bytes at or beyond out_cap"


def test_invalid_envelopes_have_no_frame(sv, orc):
    sv.set_signing_seed(SEED, 2)
    env = make_env(130, salt=5).copy()
    env[5, 0] = ord("Q")   # bad magic
    env[17, 4] = 0         # a PrePrepare's kind
    env[63, 4] = 3
    env[64, 3] = 0         # the first envelope of the second wave
    env[65, 4] = 255
    env[129, 2] ^= 1       # the last one
    stream, frame_off, sigs = E.oracle_frames(orc, SEED, 2, env)
    assert sorted(np.nonzero(np.diff(frame_off) == 0)[0].tolist()) == [5, 17, 63, 64, 65, 129]
    out, off, sig = run_device(sv, env, align=9, total=len(stream))
    assert (off == frame_off).all() and (sig == sigs).all() and (out[:len(stream)] == stream).all()
    assert (out[len(stream):] == POISON).all()
    got = sv.sign_votes_frames(env)  # the blocking form computes the same layout on the host
    assert (got[0] == stream).all() and (got[1] == frame_off).all() and (got[2] == sigs).all()


def test_round_trip_through_the_ingress_chain(sv, orc):
    """64 signers x 16 envelopes (8 seqs, both kinds): the emitted streams, one connection per signer, go into
    verify_streams_tally with the signers' keys installed."""
    n_sig, seqs = 64, 8
    seeds = seeds_for(n_sig, tag=77)
    d = np.stack([np.frombuffer(hashlib.blake2b(b"op-%d" % q, digest_size=64).digest(), np.uint8)
                  for q in range(seqs) for _ in (1, 2)])
    env = E.envelopes([1, 2] * seqs, [1] * (2 * seqs), np.repeat(np.arange(1, seqs + 1), 2), d)
    keys, streams = [], []
    try:
        for k in range(n_sig):
            keys.append(sv.set_signing_seed(seeds[k].tobytes(), k))
            streams.append(sv.sign_votes_frames(env, with_sigs=False)[0])
    finally:
        sv.set_signing_seed(SEED, 2)
    assert sv.set_keys(np.stack(keys)).all()
    lens = np.array([len(s) for s in streams], np.uint64)
    res = sv.verify_streams_tally(np.concatenate(streams), np.cumsum(lens) - lens, lens, frame_cap=n_sig * len(env) + 8,
                                  env_cap=64, seg_peer=np.arange(n_sig, dtype=np.uint16))
    n = n_sig * len(env)
    assert res["n"] == n and int(res["n_env"][0]) == len(env)
    bits = np.unpackbits(res["bitmap"].view(np.uint8), bitorder="little")[:n]
    assert bits.all(), np.nonzero(bits == 0)[0][:8]
    assert (res["counts"][:len(env)] == n_sig).all() and (res["signers"][:len(env)] == np.uint64(2**64 - 1)).all()
    assert (res["envelopes"][:len(env)] == env).all()


def test_capture_and_replay(sv, orc):
    import torch
    sv.set_signing_seed(SEED, 2)
    n, dev = 200, torch.device("cuda", 0)
    refs = [reference(orc, n, 2, salt=s) for s in (0, 11, 12)]
    cap = max(len(r[1]) for r in refs) + 64
    sv.egress_reserve(n)
    d_env = torch.from_numpy(refs[0][0].reshape(-1).copy()).to(dev)
    d_out = torch.full((cap + GUARD,), POISON, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_sig = torch.zeros(64 * n, dtype=torch.uint8, device=dev)
    args = (d_env.data_ptr(), n, d_out.data_ptr() + 1, cap, d_off.data_ptr(), d_sig.data_ptr())
    sv.sign_votes_frames_device(*args)  # (an eager call first: the kernels are loaded)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sv.sign_votes_frames_device(*args, stream=torch.cuda.current_stream().cuda_stream)
    for env, stream, frame_off, sigs in refs[1:] + refs[:1]:
        d_env.copy_(torch.from_numpy(env.reshape(-1).copy()))
        d_out.fill_(POISON)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()[1:]
        assert (d_off.cpu().numpy().view(np.uint64) == frame_off).all()
        assert (d_sig.cpu().numpy().reshape(n, 64) == sigs).all()
        assert (out[:len(stream)] == stream).all() and (out[len(stream):] == POISON).all()


def test_gpu_replica_against_the_cpu_signer(orc):
    """n = 4, 16 seqs through push_streams: the replica that signs on the GPU emits the bytes its twin emits through the
    oracle override, and with the loopback both report the same events after the next flush."""
    from pbft_amd import GpuBatchVerifier, wire
    from replica_sim import EV_PRE_PREPARED, EV_PREPARED, KIND_PREPARE, KIND_PREPREPARE, Cluster, Event
    from test_replica_streams import SegHead, bind as bind_streams
    c = Cluster(4, use_oracle_verifier=False)
    L = bind_streams(E.bind(c.L))
    gvs = [GpuBatchVerifier(0), GpuBatchVerifier(0)]
    reps, me, view, seqs = [], 2, 1, list(range(1, 17))
    op = b"testOperation"
    D = hashlib.blake2b(op, digest_size=64).digest()
    try:
        for g in gvs:
            assert g.set_keys(c.keys_np.reshape(4, 32)).all()
            r = ctypes.c_void_p()
            assert L.pbft_replica_create(g._ctx, 4, me, c.keys, ctypes.byref(r)) == 0
            reps.append(r)
        gpu, twin = reps
        assert L.pbft_replica_set_signing_seed(gpu, c.seeds[3]) == E.EINVAL  # another replica's seed: nothing changes
        signer = E.OracleSigner(orc, c.seeds[me])
        signer.install(L, twin)
        p = c.primary(view)
        seg = {p: b"".join(wire.encode_frame(wire.WireMsg(kind=wire.PREPREPARE, view=view, seq=q, digest=D, replica=p,
                                                          sig=c.sign(p, KIND_PREPREPARE, view, q, D), operation=op,
                                                          timestamp=q, client="127.0.0.1:8080")) for q in seqs)}
        for s, qs in ((0, seqs), (3, seqs[:8])):
            sg = np.stack([np.frombuffer(c.sign(s, KIND_PREPARE, view, q, D), np.uint8) for q in qs])
            seg[s] = wire.encode_votes([1] * len(qs), [view] * len(qs), qs, np.tile(np.frombuffer(D, np.uint8),
                                       (len(qs), 1)), [s] * len(qs), sg).tobytes()
        order = sorted(seg)
        stream = np.frombuffer(b"".join(seg[s] for s in order) + bytes(16), np.uint8).copy()
        length = np.array([len(seg[s]) for s in order], np.uint64)
        off = (np.cumsum(length) - length).astype(np.uint64)
        peer = np.array(order, np.uint16)

        def push(r, n_seg):
            heads = (SegHead * 4)()
            a, b, ne, ev = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32(), (Event * 256)()
            assert L.pbft_replica_push_streams(r, stream.ctypes.data, int(length[:n_seg].sum()), off.ctypes.data,
                                               length.ctypes.data, peer.ctypes.data, n_seg, heads, ctypes.byref(a),
                                               ctypes.byref(b), ev, 256, ctypes.byref(ne)) == 0
            return [(e.view, e.seq, e.kind) for e in ev[:ne.value]]

        first = push(gpu, 3)  # before any signer: the same events, nothing queued
        assert E.egress_stats(L, gpu)["queued"] == 0
        assert L.pbft_replica_destroy(gpu) == 0
        assert L.pbft_replica_create(gvs[0]._ctx, 4, me, c.keys, ctypes.byref(reps[0])) == 0
        gpu = reps[0]
        assert L.pbft_replica_set_signing_seed(gpu, c.seeds[me]) == 0
        events = [push(r, 3) for r in (gpu, twin)]
        assert events[0] == events[1] == first
        assert sum(k == EV_PRE_PREPARED for _, _, k in first) == 16 and sum(k == EV_PREPARED for _, _, k in first) == 8
        outs = [E.emit(L, r, flags=E.EMIT_LOOPBACK) for r in (gpu, twin)]
        assert outs[0][0] == outs[1][0] == 0 and outs[0][3] == outs[1][3] == 24
        assert outs[0][1].tobytes() == outs[1][1].tobytes()
        v = wire.decode_votes(outs[0][1].tobytes(), 4)
        assert (v.status == 0).all() and (v.key_idx == me).all() and len(v.R) == 24
        after = [push(r, 0) for r in (gpu, twin)]  # the own Prepares complete seqs 9..16
        assert after[0] == after[1] == [(view, q, EV_PREPARED) for q in seqs[8:]]
        st = [E.egress_stats(L, r) for r in (gpu, twin)]
        assert all((s["emitted"], s["loopback_pushed"], s["queued"]) == (24, 24, 8) for s in st)
    finally:
        for r in reps:
            L.pbft_replica_destroy(r)
        for g in gvs:
            g.close()
        c.close()
