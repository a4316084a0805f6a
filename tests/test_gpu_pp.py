"""The residue's PrePrepares on the GPU: pbft_wire_decode_preprepares_device against the host build of the same rule
(pbft_wire_decode_preprepare) head for head, the chain pbft_verify_streams_admit_pp against pbft_verify_streams_admit,
the replica differential of tests/test_gpu_replica_streams.py on PrePrepare traffic with no digest override -- so the
device's `computed` is what gates the windows -- and one capture and replay."""

import numpy as np
import pytest

import pp_traffic as P
import streams_traffic as T
from test_gpu_frames import GUARD, dev_bytes
from test_gpu_replica_streams import GpuPair, gvs  # noqa: F401  (fixture)
from test_gpu_verify import gv, seeds_for  # noqa: F401  (fixture)
from test_pp import SEQS, count_pp, pp_stats, set_pp

pytestmark = pytest.mark.gpu
POISON = 0xA5


def host_head(body):
    from pbft_amd import wire
    return wire.decode_preprepare(body)


def lay_out(bodies, tail_entries=()):
    """The bodies in one stream, body k at an offset with off % 16 == k % 16, the last one ending on the stream's last
    byte with a partial final granule; -> (stream, residue entries)."""
    from pbft_amd.wire import AdmitResidue
    parts, at, res = [], 0, []
    for k, b in enumerate(bodies):
        gap = (k % 16 - at) % 16
        if k == len(bodies) - 1 and (at + gap + len(b)) % 16 == 0:
            gap += 16 + 5  # (keeps the final granule partial; this body's alignment is covered by an earlier one)
        parts += [b"\x7b" * gap, b]
        res.append((at + gap, k, len(b)))
        at += gap + len(b)
    stream = np.frombuffer(b"".join(parts), np.uint8).copy()
    assert len(stream) % 16 != 0 and res[-1][0] + res[-1][2] == len(stream)
    return stream, np.array(res + list(tail_entries), AdmitResidue)


def run_device(gv, stream, res, cap, n_res="null", pad_entries=0):
    """One call on its own stream over poisoned heads; -> the cap heads (the guard behind them checked)."""
    import torch
    from pbft_amd._lib import check, load
    from pbft_amd.wire import PpHead
    d_stream = dev_bytes(stream, pad=(-len(stream)) % 16)
    assert d_stream.data_ptr() % 16 == 0
    d_res = dev_bytes(np.concatenate([res, np.zeros(pad_entries, res.dtype)])) if len(res) + pad_entries else None
    d_n = dev_bytes(np.array([n_res, 0], np.uint32)) if n_res != "null" else None
    d_pp = torch.full((cap * 232 + GUARD,), POISON, dtype=torch.uint8, device=torch.device("cuda", 0))
    ts = torch.cuda.Stream()
    check(load().pbft_wire_decode_preprepares_device(gv._ctx, d_stream.data_ptr(), len(stream),
                                                     d_res.data_ptr() if d_res is not None else d_pp.data_ptr(),
                                                     d_n.data_ptr() if d_n is not None else None, cap,
                                                     d_pp.data_ptr(), ts.cuda_stream))
    ts.synchronize()
    a = d_pp.cpu().numpy()
    assert (a[cap * 232:] == POISON).all(), "guard behind the heads overwritten"
    return a[:cap * 232].view(PpHead).copy()


@pytest.fixture(scope="module")
def chosen():
    """The CPU corpus's accepted frames and every 40th of the others, with their host heads."""
    from pbft_amd import wire
    corpus = P.corpus()
    heads = [host_head(b) for b, _ in corpus]
    ok = [k for k, h in enumerate(heads) if h["status"] == wire.PP_OK]
    no = [k for k, h in enumerate(heads) if h["status"] != wire.PP_OK][::40]
    pick = sorted(ok + no)
    assert len(ok) > 30 and len(no) > 300
    return [corpus[k][0] for k in pick], np.array([heads[k] for k in pick])


def test_kernels_against_the_host_rule(gv, chosen):
    from pbft_amd import wire
    bodies, want = chosen
    n = len(bodies)
    assert {k % 16 for k in range(n) if want[k]["status"] == wire.PP_OK} == set(range(16))
    outside = [(0, n, 0), (1, n + 1, 500), (2**40, n + 2, 400), (2**64 - 200, n + 3, 400)]
    stream, res = lay_out(bodies)
    outside[1] = (len(stream) - 10, n + 1, 500)  # begins inside the stream, ends behind it
    stream, res = lay_out(bodies, outside)
    got = run_device(gv, stream, res, len(res))
    bad = [k for k in range(n) if got[k].tobytes() != want[k].tobytes()]
    assert not bad, (bad[:8], got[bad[0]], want[bad[0]])
    assert got[n:].tobytes() == bytes(232 * len(outside))
    assert int((got["status"] == wire.PP_OK).sum()) == int((want["status"] == wire.PP_OK).sum()) > 30


def test_last_frame_on_the_last_byte(gv, chosen):
    """An accepted frame that ends on the stream's last byte, inside a partial granule."""
    from pbft_amd import wire
    bodies, want = chosen
    ok = [k for k in range(len(bodies)) if want[k]["status"] == wire.PP_OK]
    pick = [bodies[k] for k in ok[:5]]
    stream, res = lay_out(pick)
    got = run_device(gv, stream, res, len(res))
    assert got.tobytes() == want[ok[:5]].tobytes() and got[-1]["status"] == wire.PP_OK


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 130, "null"])
def test_residue_counts(gv, chosen, count):
    """residue_cap = 128: entries below min(count, 128) get their heads, the others are zeroed; 130 writes 128."""
    from pbft_amd import wire
    bodies, want = chosen
    ok = [k for k in range(len(bodies)) if want[k]["status"] == wire.PP_OK and len(bodies[k]) < 700]
    pick = [ok[i % len(ok)] if i % 3 else i % len(bodies) for i in range(130)]
    stream, res = lay_out([bodies[k] for k in pick])
    cap = 128
    got = run_device(gv, stream, res[:cap], cap, n_res=count)
    live = cap if count == "null" else min(count, cap)
    exp = want[pick[:cap]].copy()
    exp[live:] = np.zeros(1, exp.dtype)
    assert got.tobytes() == exp.tobytes()
    if live:
        assert (got[:live]["status"] == wire.PP_OK).any()


def test_arguments(gv):
    from pbft_amd import load
    lib = load()
    import torch
    t = torch.zeros(4096, dtype=torch.uint8, device=torch.device("cuda", 0))
    p = t.data_ptr()
    call = lib.pbft_wire_decode_preprepares_device
    assert call(gv._ctx, p, 1024, p + 1024, None, 4, p + 2048, None) == 0
    torch.cuda.synchronize()
    assert call(gv._ctx, p + 8, 1024, p + 1024, None, 4, p + 2048, None) == -1   # stream not 16-byte aligned
    assert call(gv._ctx, p, 1024, p + 1028, None, 4, p + 2048, None) == -1       # residue not 8-byte aligned
    assert call(gv._ctx, p, 1024, p + 1024, None, 4, p + 2052, None) == -1       # heads not 8-byte aligned
    assert call(gv._ctx, p, 1024, p + 1024, p + 1026, 4, p + 2048, None) == -1   # count not 4-byte aligned
    assert call(gv._ctx, p, 2**31 + 1, p + 1024, None, 4, p + 2048, None) == -1  # stream_bytes out of range
    assert call(gv._ctx, None, 1024, p + 1024, None, 4, p + 2048, None) == -1
    assert call(gv._ctx, p, 1024, None, None, 4, p + 2048, None) == -1
    assert call(gv._ctx, p, 1024, p + 1024, None, 4, None, None) == -1
    torch.cuda.synchronize()
    assert not t.cpu().numpy()[2048 + 4 * 232:].any()  # the refused calls wrote nothing


# ---- the chain ----
class Chain:
    """pbft_verify_streams_admit / _pp over one call's bytes, every output poisoned first."""

    def __init__(self, gv, n, frame_cap=2048, env_cap=128, residue_cap=1024):
        from pbft_amd import load
        from pbft_amd.wire import AdmitResidue, PpHead, SegHead
        self.gv, self.n, self.lib = gv, n, load()
        self.caps = (frame_cap, env_cap, residue_cap)
        self.W = (n + 63) // 64
        self.dt = dict(seg=SegHead, res=AdmitResidue, pp=PpHead)

    def run(self, call, pp):
        stream, off, length, peer = call
        fc, ec, rc = self.caps
        S = len(off)
        o = dict(seg=np.zeros(S, self.dt["seg"]), n_frames=np.zeros(2, np.uint32), counts=np.zeros(8, np.uint32),
                 env=np.zeros(ec * 85, np.uint8), n_env=np.zeros(2, np.uint32), present=np.zeros(ec * self.W, np.uint64),
                 valid=np.zeros(ec * self.W, np.uint64), res=np.zeros(rc, self.dt["res"]), n_res=np.zeros(2, np.uint32))
        for a in o.values():
            a.view(np.uint8)[:] = POISON
        args = [self.gv._ctx, stream.ctypes.data, len(stream), off.ctypes.data, length.ctypes.data, peer.ctypes.data, S,
                self.n, fc, ec, rc, T.VIEW, 0, T.WINDOW] + [o[k].ctypes.data for k in o]
        if pp:
            o["pp"] = np.zeros(rc, self.dt["pp"])
            o["pp"].view(np.uint8)[:] = POISON
            rcode = self.lib.pbft_verify_streams_admit_pp(*args, o["pp"].ctypes.data)
        else:
            rcode = self.lib.pbft_verify_streams_admit(*args)
        assert rcode == 0, rcode
        return o


@pytest.mark.parametrize("n", [4, 16])
def test_chain_against_the_old_call(gv, n):
    """Output for output equal to pbft_verify_streams_admit on the same bytes, the heads equal to the host rule; a call
    without a deferred frame returns without touching pp_out."""
    from pbft_amd import wire
    seeds = seeds_for(n, tag=n)

    def sign_batch(signers, env):
        R, S, pub = gv.sign(seeds, signers, env, 85)
        if not sign_batch.keys:
            assert gv.set_keys(pub).all()
            sign_batch.keys = True
        return np.concatenate([R, S], axis=1)
    sign_batch.keys = False
    named = P.kinds(n, SEQS)
    calls = T.materialize(T.together(named) + [[s for s in named["honest"][1]]], sign_batch)
    ch = Chain(gv, n)
    seen_pp = 0
    for k, call in enumerate(calls):
        old, new = ch.run(call, False), ch.run(call, True)
        for key in old:  # (the envelope table is defined up to n_env)
            cut = int(new["n_env"][0]) * 85 if key == "env" else None
            assert old[key][:cut].tobytes() == new[key][:cut].tobytes(), (k, key)
        assert new["n_res"][0] <= ch.caps[2] and new["n_frames"][0] <= ch.caps[0] and new["n_env"][0] <= ch.caps[1]
        live = int(new["n_res"][0])
        raw = new["pp"].view(np.uint8).reshape(-1, 232)
        if new["counts"][5] == 0:  # PBFT_ADMIT_HOST
            assert (raw == POISON).all(), k
            continue
        assert (raw[live:] == POISON).all(), k
        stream = call[0].tobytes()
        for i in range(live):
            e = new["res"][i]
            want = host_head(stream[int(e["off"]):int(e["off"]) + int(e["len"])])
            assert new["pp"][i].tobytes() == want.tobytes(), (k, i)
            seen_pp += int(want["status"] == wire.PP_OK)
    assert seen_pp > 20
    assert calls and ch.run(calls[-1], True)["counts"][5] == 0  # the last call is votes only


# ---- the replica, on real signatures, no digest override ----
@pytest.mark.parametrize("on", [1, 0])
@pytest.mark.parametrize("n", [4, 16])
def test_replica_differential(gvs, n, on):  # noqa: F811
    named = P.kinds(n, SEQS)
    runs = list(named.items()) + [("together", T.together(named))]
    if n == 16:  # (every kind alone at n = 4; at 16 the honest rounds and all kinds merged)
        runs = [r for r in runs if r[0] in ("honest", "together")]
    for name, calls in runs:
        p = GpuPair(gvs, n)
        try:
            set_pp(p, on)
            p.run(calls, name)
            s = p.sstats()
            assert s["calls_device"] == len(calls) and s["calls_host_front"] == 0, (name, s)
            assert not any(v for k, v in s.items() if k.startswith("fallback_")), (name, s)
            canon, other = count_pp(calls)
            assert canon > 0
            assert pp_stats(p, p.B) == ((canon, other) if on else (0, canon + other)), name
            if name in ("honest", "escaped operation", "between votes"):
                assert all(p.L.pbft_replica_committed_local(p.B, T.VIEW, q) == 1 for q in SEQS), name
        finally:
            p.close()


def test_capture_and_replay(gv, chosen):
    """The device call captured into a graph (a plain chain of kernel nodes) and replayed on other bytes."""
    import torch
    from pbft_amd import wire
    from pbft_amd._lib import check, load
    from pbft_amd.wire import PpHead
    bodies, want = chosen
    ok = [k for k in range(len(bodies)) if want[k]["status"] == wire.PP_OK and len(bodies[k]) < 700]
    sets = [[ok[(3 * i + r) % len(ok)] if (i + r) % 4 else (7 * i + r) % len(bodies) for i in range(40)] for r in range(3)]
    laid = [lay_out([bodies[k] for k in s]) for s in sets]
    size = max(len(s) for s, _ in laid) + 32
    cap = 48  # 40 live entries, 8 behind the count
    d_stream = torch.zeros(size, dtype=torch.uint8, device=torch.device("cuda", 0))
    d_res, d_n = dev_bytes(np.zeros(cap, laid[0][1].dtype)), dev_bytes(np.array([40, 0], np.uint32))
    d_pp = torch.full((cap * 232 + GUARD,), POISON, dtype=torch.uint8, device=torch.device("cuda", 0))
    lib = load()

    def enqueue(stream):
        # (stream_bytes is a launch argument: the graph keeps the largest, every entry is tested against it)
        check(lib.pbft_wire_decode_preprepares_device(gv._ctx, d_stream.data_ptr(), size - 32, d_res.data_ptr(),
                                                      d_n.data_ptr(), cap, d_pp.data_ptr(), stream))
    enqueue(None)  # (an eager call first: the kernels are loaded)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        enqueue(torch.cuda.current_stream().cuda_stream)
    for s, (stream, res) in zip(sets, laid):
        d_stream.zero_()
        d_stream[:len(stream)].copy_(dev_bytes(stream))
        d_res[:16 * 40].copy_(dev_bytes(res))
        d_pp.fill_(POISON)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        a = d_pp.cpu().numpy()
        assert (a[cap * 232:] == POISON).all()
        got = a[:cap * 232].view(PpHead)
        assert got[:40].tobytes() == want[s].tobytes() and got[40:].tobytes() == bytes(8 * 232)
        assert (got["status"] == wire.PP_OK).sum() > 20
