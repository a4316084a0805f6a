"""Client replies on the GPU: pbft_sign_replies(_device) byte for byte against hashlib's digests over C | result, the C
oracle's RFC 8032 signatures over pbft_reply_envelope and pbft_wire_encode_replies (tests/reply_sim.py) -- the stream,
reply_off, the digests, the signatures and the status -- over poisoned outputs with guards in front of and behind every
buffer; then one capture and replay, the client's round trip through pbft_wire_decode_reply and pbft_verify_batch, and a
GPU replica's pbft_replica_reply against a twin that replies through the CPU override."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import egress_sim as E
import reply_sim as R
from conftest import ROOT
from pbft_amd import wire
from test_gpu_verify import gv  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
POISON, GUARD = 0xA5, 512
SEED = hashlib.sha512(b"reply-seed").digest()[:32]
VIEW = 10**19 - 1  # 19 digits


@pytest.fixture(scope="module")
def orc():
    o = ctypes.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))
    o.oracle_public_key.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    return E.bind_oracle(o)


@pytest.fixture(scope="module")
def L():
    return R.bind(wire.load())


@pytest.fixture(scope="module")
def sv(gv, orc):  # noqa: F811
    """The module's verifier with SEED installed as replica 2."""
    assert gv.set_signing_seed(SEED, 2).tobytes() == R.public_key(orc, SEED)
    yield gv
    gv.set_signing_seed(None)


_ref = {}


def reference(L, orc, n, salt=0, replica=2, view=VIEW, general=True):
    """dict: the executed requests and everything both forms must return for them (computed once per key, never
    changed)."""
    key = (n, salt, replica, view, general)
    if key not in _ref:
        res, ts, cl = R.mixed_results(n, salt, general)
        req, stream, off, dig, sig, st = R.reference(L, orc, SEED, replica, view, res, ts, cl)
        dev, dev_off = R.device_reference(stream, off, st)
        _ref[key] = dict(res=res, ts=ts, cl=cl, req=req, stream=stream, off=off, dig=dig, sig=sig, st=st, dev=dev,
                         dev_off=dev_off, view=view)
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


def run_device(v, req, n, view=VIEW, align=0, cap=0, results_bytes=None, poison_behind=False):
    """One device call over poisoned outputs -> (out [cap], reply_off, digests, sigs, status), every guard checked.
    poison_behind: the results' buffer holds POISON from results_bytes on (the reader must not let it into D)."""
    import torch
    dev = torch.device("cuda", 0)
    data, nb, off, ln, ts, cl = req
    nb = nb if results_bytes is None else results_bytes
    if poison_behind:
        data = np.concatenate([data[:nb], np.full(64, POISON, np.uint8)])
    ins = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy() if a.size else
                            np.zeros(16, np.uint8)).to(dev) for a in (data, off, ln, ts, cl)]
    d_out, d_off = guarded(torch, dev, cap, align), guarded(torch, dev, 8 * (n + 1))
    d_dig, d_sig, d_st = guarded(torch, dev, 64 * n), guarded(torch, dev, 64 * n), guarded(torch, dev, n)
    s = torch.cuda.Stream()
    p = [t.data_ptr() for t in ins]
    assert p[0] % 16 == 0
    v.sign_replies_device(p[0], nb, p[1], p[2], p[3], p[4], view, n, d_out.data_ptr() + GUARD + align, cap,
                          d_off.data_ptr() + GUARD, d_dig.data_ptr() + GUARD, d_sig.data_ptr() + GUARD,
                          d_st.data_ptr() + GUARD, stream=s.cuda_stream)
    s.synchronize()
    return (body(d_out, cap, align), body(d_off, 8 * (n + 1)).copy().view(np.uint64),
            body(d_dig, 64 * n).reshape(n, 64), body(d_sig, 64 * n).reshape(n, 64), body(d_st, n))


def check_exact(v, r, align=0, slack=64, **kw):
    n = len(r["st"])
    total = len(r["dev"])
    out, off, dig, sig, st = run_device(v, r["req"], n, view=r["view"], align=align, cap=total + slack, **kw)
    assert (st == r["st"]).all(), np.nonzero(st != r["st"])[0][:8]
    assert (off == r["dev_off"]).all(), np.nonzero(off != r["dev_off"])[0][:8]
    assert (dig == r["dig"]).all(), np.nonzero((dig != r["dig"]).any(axis=1))[0][:8]
    assert (sig == r["sig"]).all(), np.nonzero((sig != r["sig"]).any(axis=1))[0][:8]
    bad = np.nonzero(out[:total] != r["dev"])[0]
    assert bad.size == 0, (bad[:8], int(np.searchsorted(r["dev_off"], bad[0], side="right")) - 1)
    assert (out[total:] == POISON).all(), "bytes behind reply_off[N] overwritten"


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 130])
def test_byte_exact(sv, orc, L, n):
    """Digests against hashlib, signatures against the oracle's signer over pbft_reply_envelope, texts against
    pbft_wire_encode_replies."""
    r = reference(L, orc, n)
    if n >= 63:
        assert 0 < int((r["st"] == 0).sum()) < n  # general results among canonical ones
        lens = {len(x) for x, s in zip(r["res"], r["st"]) if s == 0}
        assert lens >= {0, 1, 63, 64, 65, 191, 192, 193, 3071, 3072}  # the block boundaries inside one wave
    if n == 130:  # general: too long and non-alphabet; no text, digest and signature still right
        gen = [x for x, s in zip(r["res"], r["st"]) if s == 1]
        assert any(len(x) == 3073 and wire.reply_canonical(x[:3072]) for x in gen)
        assert any(len(x) <= 3072 for x in gen)
        assert (np.diff(r["dev_off"].astype(np.int64))[r["st"] == 1] == 0).all()
    check_exact(sv, r, align=n % 16)


@pytest.mark.parametrize("align", range(16))
def test_every_alignment_of_the_output(sv, orc, L, align):
    check_exact(sv, reference(L, orc, 65, salt=1), align=align)


@pytest.mark.parametrize("shift", range(4))
@pytest.mark.parametrize("tail", [1, 2, 3])
def test_every_alignment_of_a_result_and_the_end_of_the_results(sv, orc, L, shift, tail):
    """A first result of `shift` bytes moves every other result through the four alignments; the last result ends at
    results_bytes = tail mod 4, the bytes behind hold poison and must not change D."""
    key = ("shifted", shift, tail)
    if key not in _ref:
        res, ts, cl = R.mixed_results(22, salt=2, general=False)
        res = [b"s" * shift] + res + [b"z" * 61]
        ts, cl = [7] + ts + [8], [b"c"] + cl + [b"127.0.0.1:8080"]
        while sum(len(x) for x in res) % 4 != tail:
            res[-1] += b"z"
        req, stream, off, dig, sig, st = R.reference(L, orc, SEED, 2, VIEW, res, ts, cl)
        dev, dev_off = R.device_reference(stream, off, st)
        _ref[key] = dict(res=res, req=req, stream=stream, off=off, dig=dig, sig=sig, st=st, dev=dev, dev_off=dev_off,
                         view=VIEW)
    r = _ref[key]
    assert r["req"][1] % 4 == tail and int(r["req"][2][-1]) + int(r["req"][3][-1]) == r["req"][1]
    check_exact(sv, r, align=shift, poison_behind=True)


@pytest.mark.parametrize("cut", ["mid_reply_mid_wave", "reply_boundary", "wave_boundary", "first_reply", "zero"])
def test_short_output(sv, orc, L, cut):
    """out_cap inside the stream: the replies that fit are exact, nothing at or beyond out_cap is written (nor between
    the last whole reply and out_cap), and reply_off, digests, sigs and status are complete."""
    r = reference(L, orc, 130)
    fo = r["dev_off"]
    ok = np.nonzero(r["st"] == 0)[0]
    a, b = int(ok[ok > 70][0]), int(ok[ok > 70][1])  # two canonical replies of the second wave
    fit, cap = {"mid_reply_mid_wave": (a, int(fo[a]) + 100), "reply_boundary": (b, int(fo[b])),
                "wave_boundary": (64, int(fo[64])), "first_reply": (0, 200), "zero": (0, 0)}[cut]
    assert int(r["st"][0]) == 0 and int(fo[1]) > 200
    out, off, dig, sig, st = run_device(sv, r["req"], 130, align=7, cap=cap)
    end = int(fo[fit])
    assert (off == fo).all() and int(off[-1]) == len(r["dev"]) > cap
    assert (dig == r["dig"]).all() and (sig == r["sig"]).all() and (st == r["st"]).all()
    assert (out[:end] == r["dev"][:end]).all()
    assert (out[end:] == POISON).all(), "a reply written in part, or bytes at or beyond out_cap"


def test_result_outside_results_bytes(sv, orc, L):
    """Such a reply is not read: zero digest and signature, status GENERAL, its neighbours unaffected."""
    r = reference(L, orc, 65, salt=2)
    data, nb, off, ln, ts, cl = r["req"]
    off2, ln2 = off.copy(), ln.copy()
    off2[3] = nb - 1           # ends one byte behind results_bytes
    ln2[3] = 2
    off2[64] = 2**63           # far outside
    ln2[40] = 2**32 - 1        # longer than everything
    out, roff, dig, sig, st = run_device(sv, (data, nb, off2, ln2, ts, cl), 65, cap=len(r["dev"]) + 64)
    want_st, want_dig, want_sig = r["st"].copy(), r["dig"].copy(), r["sig"].copy()
    for i in (3, 40, 64):
        want_st[i], want_dig[i], want_sig[i] = 1, 0, 0
    assert (st == want_st).all() and (dig == want_dig).all() and (sig == want_sig).all()
    lens = np.diff(r["dev_off"].astype(np.int64))
    lens[[3, 40, 64]] = 0
    assert (roff == np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)).all()
    keep = [i for i in range(65) if want_st[i] == 0]
    want = np.concatenate([r["dev"][int(r["dev_off"][i]):int(r["dev_off"][i + 1])] for i in keep])
    assert (out[:len(want)] == want).all() and (out[len(want):] == POISON).all()
    from pbft_amd import PbftError
    with pytest.raises(PbftError) as e:  # the blocking form refuses it
        sv.sign_replies(VIEW, (data, nb, off2, ln2, ts, cl))
    assert e.value.code == -1


@pytest.mark.parametrize("replica,view", [(0, 0), (65534, 2**64 - 1)])
def test_replica_index_and_number_widths(sv, orc, L, replica, view):
    """Replica 0 and 65,534; view of width 1 and 20; the timestamps walk every width edge (R.VALS: 0 and 2^64 - 1)."""
    sv.set_signing_seed(SEED, replica)
    try:
        r = reference(L, orc, 65, salt=3, replica=replica, view=view)
        assert {0, 2**64 - 1} <= set(r["ts"])
        check_exact(sv, r, align=3)
    finally:
        sv.set_signing_seed(SEED, 2)


def test_arguments_and_a_clone_without_a_seed(sv, orc, L):
    from pbft_amd import PbftError
    r = reference(L, orc, 7, salt=5)
    c = sv.clone()  # a clone does not inherit the seed: replying without one is PBFT_EINVAL
    try:
        with pytest.raises(PbftError) as e:
            c.sign_replies(VIEW, r["req"])
        assert e.value.code == -1
        with pytest.raises(PbftError) as e:
            run_device(c, r["req"], 7, cap=1 << 16)
        assert e.value.code == -1
        c.set_signing_seed(SEED, 2)
        assert (c.sign_replies(VIEW, r["req"])[0] == r["stream"]).all()
    finally:
        c.close()
    with pytest.raises(PbftError):
        sv.reply_reserve(2**24 + 1)
    # a short cap: PBFT_EINVAL with the length, the offsets and the status; nothing launched
    data, nb, off, ln, ts, cl = r["req"]
    need = ctypes.c_size_t()
    roff, st = np.zeros(8, np.uint64), np.full(7, 9, np.uint8)
    out = np.full(len(r["stream"]), POISON, np.uint8)
    rc = wire.load().pbft_sign_replies(sv._ctx, data.ctypes.data, nb, off.ctypes.data, ln.ctypes.data, ts.ctypes.data,
                                       cl.ctypes.data, VIEW, 7, out.ctypes.data, len(out) - 1, ctypes.byref(need),
                                       roff.ctypes.data, None, None, st.ctypes.data)
    assert rc == -1 and need.value == len(r["stream"]) and (roff == r["off"]).all() and (st == r["st"]).all()
    assert (out == POISON).all()


@pytest.mark.parametrize("n,salt", [(130, 0), (65, 4), (7, 5), (0, 0)])
def test_blocking_form(sv, orc, L, n, salt):
    """Equal to encode_replies on the mixed input: the general results' texts are made on the host from the device's
    signatures."""
    r = reference(L, orc, n, salt)
    stream, off, dig, sig, st = sv.sign_replies(VIEW, r["req"])
    assert (st == r["st"]).all() and (off == r["off"]).all() and (dig == r["dig"]).all() and (sig == r["sig"]).all()
    assert len(stream) == len(r["stream"]) and (stream == r["stream"]).all()


def test_blocking_form_all_canonical(sv, orc, L):
    r = reference(L, orc, 70, salt=6, general=False)
    got = sv.sign_replies(VIEW, r["req"])
    assert (r["st"] == 0).all() and (got[0] == r["stream"]).all() and (got[1] == r["off"]).all()
    assert (got[2] == r["dig"]).all() and (got[3] == r["sig"]).all()


def test_capture_and_replay(sv, orc, L):
    """The three launches as one hipGraph: a plain chain."""
    import torch
    n, dev = 130, torch.device("cuda", 0)
    # is stream capture available at all?  Asked with one trivial torch operation, before any of the project's code runs
    probe_t = torch.zeros(16, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    try:
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            probe_t.add_(1)
    except RuntimeError as e:
        pytest.skip("stream capture refused: %s" % e)
    refs = [reference(L, orc, n, salt=s) for s in (0, 11, 12)]
    cap = max(len(r["dev"]) for r in refs) + 64
    size = [max(a[k].nbytes for a in (r["req"] for r in refs)) for k in (0, 2, 3, 4, 5)]
    nb = max(r["req"][1] for r in refs)
    assert all(r["req"][1] == nb for r in refs)  # (the mixes differ in bytes, not in lengths)
    sv.reply_reserve(n)
    d_in = [torch.zeros(s + 16, dtype=torch.uint8, device=dev) for s in size]
    d_out = torch.full((cap + GUARD,), POISON, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_dig, d_sig = (torch.zeros(64 * n, dtype=torch.uint8, device=dev) for _ in range(2))
    d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
    p = [t.data_ptr() for t in d_in]
    args = (p[0], nb, p[1], p[2], p[3], p[4], VIEW, n, d_out.data_ptr() + 1, cap, d_off.data_ptr(), d_dig.data_ptr(),
            d_sig.data_ptr(), d_st.data_ptr())

    def load(r):
        data, _, off, ln, ts, cl = r["req"]
        for t, a in zip(d_in, (data, off, ln, ts, cl)):
            b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
            t[:len(b)].copy_(torch.from_numpy(b.copy()))

    load(refs[0])
    sv.sign_replies_device(*args)  # (an eager call first: the kernels are loaded)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # (an error of the call under capture fails the test)
        sv.sign_replies_device(*args, stream=torch.cuda.current_stream().cuda_stream)
    for r in refs[1:] + refs[:1]:
        load(r)
        d_out.fill_(POISON)
        d_off.fill_(-1)
        d_dig.fill_(POISON), d_sig.fill_(POISON), d_st.fill_(POISON)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()[1:]
        assert (d_off.cpu().numpy().view(np.uint64) == r["dev_off"]).all()
        assert (d_dig.cpu().numpy().reshape(n, 64) == r["dig"]).all()
        assert (d_sig.cpu().numpy().reshape(n, 64) == r["sig"]).all()
        assert (d_st.cpu().numpy() == r["st"]).all()
        assert (out[:len(r["dev"])] == r["dev"]).all() and (out[len(r["dev"]):] == POISON).all()


def test_round_trip_as_a_client(sv, orc, L):
    """What a client does with the bytes: decode each reply, take the key from its peer_id text, rebuild the envelope
    from its own address and the result, and verify the batch on the GPU.  Every bit is 1; with one result byte or the
    client field changed, exactly that bit is 0."""
    from pbft_amd import GpuBatchVerifier, SigBatch, bitmap_to_bool
    r = reference(L, orc, 70, salt=6, general=False)
    stream, off, _, _, st = sv.sign_replies(VIEW, r["req"])
    n = 70
    heads = [wire.decode_reply(stream[int(off[i]):int(off[i + 1])].tobytes()) for i in range(n)]
    assert all(int(h["status"]) == wire.RH_OK for h in heads)
    A = ctypes.create_string_buffer(32)
    assert L.pbft_key_from_peer_id_b58(bytes(heads[0]["peer_id"]), 52, A) == 0 and A.raw == R.public_key(orc, SEED)
    assert all(bytes(h["peer_id"]) == bytes(heads[0]["peer_id"]) for h in heads)
    results = [stream[int(off[i]) + int(h["result_off"]):int(off[i]) + int(h["result_off"]) + int(h["result_len"])].tobytes()
               for i, h in enumerate(heads)]
    assert results == r["res"]
    sigs = np.stack([h["sig"] for h in heads])
    v = GpuBatchVerifier(0)
    try:
        assert v.set_keys(np.frombuffer(A.raw, np.uint8).reshape(1, 32)).all()

        def bits(res, cl):
            dig = R.digests_of(res, cl)  # the client's own address and the result it was sent
            env = R.envelopes(L, int(heads[0]["view"]), [int(h["timestamp"]) for h in heads], dig)
            b = SigBatch(np.ascontiguousarray(sigs[:, :32]), np.ascontiguousarray(sigs[:, 32:]), np.zeros(n, np.uint16),
                         env, 85)
            return bitmap_to_bool(v.verify(b), n)

        assert bits(results, r["cl"]).all()
        res2 = list(results)
        k = next(i for i in range(5, n) if len(results[i]) > 2)
        res2[k] = res2[k][:1] + bytes([res2[k][1] ^ 1]) + res2[k][2:]
        got = bits(res2, r["cl"])
        assert not got[k] and got.sum() == n - 1
        cl2 = list(r["cl"])
        cl2[9] = b"127.0.0.1:8081" if cl2[9] != b"127.0.0.1:8081" else b"127.0.0.1:8082"
        got = bits(results, cl2)
        assert not got[9] and got.sum() == n - 1
    finally:
        v.close()


def test_gpu_replica_against_the_cpu_twin(orc):
    """n = 4, one small round to COMMITTED_LOCAL on both: the replica that hashes, signs and writes on the GPU replies
    the bytes its twin replies through the oracle override -- status, last_timestamp and stats included, with one stale
    and one uncommitted entry."""
    from pbft_amd import GpuBatchVerifier
    from replica_sim import DIGEST_FN, EV_COMMITTED, KIND_COMMIT, KIND_PREPARE, VERIFY_FN, Cluster
    c = Cluster(4, use_oracle_verifier=False)
    L = R.bind(E.bind(c.L))
    me, view, n_seq = 2, 1, 6
    g = GpuBatchVerifier(0)
    reps, cluster_reps = [], c.reps
    try:
        assert g.set_keys(c.keys_np.reshape(4, 32)).all()
        for ctx in (g._ctx, None):
            r = ctypes.c_void_p()
            assert L.pbft_replica_create(ctx, 4, me, c.keys, ctypes.byref(r)) == 0
            reps.append(r)
        gpu, twin = reps
        vf, df = VERIFY_FN(c._oracle_verify), DIGEST_FN(c._digest)
        L.pbft_replica_set_verifier(twin, vf, None)
        L.pbft_replica_set_digest_fn(twin, df, None)
        c.reps = [gpu, twin]  # (Cluster.flush and .pre_prepare address replicas by position)
        for pos in (0, 1):
            for q in range(1, n_seq + 1):
                op = b"op-%d" % q
                assert c.pre_prepare(pos, view, q, op) == 1
                d = hashlib.blake2b(op, digest_size=64).digest()
                for kind in (KIND_PREPARE, KIND_COMMIT):
                    for s in range(4):
                        assert L.pbft_replica_push(c.reps[pos], kind, view, q, d, s, c.sign(s, kind, view, q, d)) >= 0
        events = [sorted(sum((c.flush(pos, force=1) for _ in range(3)), [])) for pos in (0, 1)]
        assert events[0] == events[1] and all((view, q, EV_COMMITTED) in events[0] for q in range(1, n_seq + 1))
        res, ts, cl = R.mixed_results(n_seq + 2)  # canonical results of the length edges ...
        res[1], res[5] = b'a "quoted" result', res[5][:40] + b"\n" + res[5][41:]  # ... and two general ones
        ts = [3, 5, 4, 9, 10, 11, 12, 13]          # 4 is stale against 5
        seqs = [1, 2, 3, 4, n_seq + 3, 5, 6, 1]     # n_seq + 3 is not committed
        req = wire.pack_results(res, ts, cl)
        assert R.reply(L, gpu, seqs, req, cap=1 << 20)[0] == R.EINVAL  # no signer yet
        assert L.pbft_replica_set_signing_seed(gpu, c.seeds[me]) == 0
        replier = R.OracleReplier(L, c.o, c.seeds[me])
        replier.install(L, twin)
        outs = [R.reply(L, r, seqs, req) for r in (gpu, twin)]
        assert outs[0][0] == outs[1][0] == 0 and outs[0][2] == outs[1][2] and outs[0][5] == outs[1][5] == 6
        assert outs[0][1].tobytes() == outs[1][1].tobytes()
        assert (outs[0][3] == outs[1][3]).all() and list(outs[0][4]) == list(outs[1][4])
        assert outs[0][4][2] == wire.REPLY_STALE and outs[0][4][4] == wire.REPLY_NOT_COMMITTED
        assert {int(x) for x in outs[0][4]} >= {wire.REPLY_OK, wire.REPLY_GENERAL}
        assert R.last_timestamp(L, gpu) == R.last_timestamp(L, twin) == 13 and replier.calls == 1
        st = [R.reply_stats(L, r) for r in (gpu, twin)]
        assert all((s["replied"], s["calls"], s["stale"], s["not_committed"]) == (6, 1, 1, 1) for s in st)
    finally:
        for r in reps:
            L.pbft_replica_destroy(r)
        g.close()
        c.reps = cluster_reps
        c.close()
