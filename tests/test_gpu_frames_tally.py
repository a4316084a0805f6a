"""Frames in, quorums out (pbft_verify_frames_tally / pbft_verify_frames_tally_device): streams of ~2,000 frames for
n = 4 and n = 256 keys whose envelopes repeat (digests from a small pool), with forged signatures, every mutant class
and signed PrePrepares, plus one envelope with exactly 2f + 1 and one with exactly 2f valid distinct signers.
The bitmap and heads are those of verify_frames / verify_frames_device on the same input; (env_idx, envelopes, n_env)
equal group_reference over the records; (signers, count) equal tally_reference.

The device form does not settle the frames its decoder defers (the host form does that, on the host): there the
yardstick is verify_frames_device -- bitmap word for word, heads and records -- and verify_frames on every frame the
device settled; its deferred frames have key index 0xFFFF and take part in no envelope."""
import numpy as np
import pytest

from test_gpu_frames import EDEFER, GUARD, DeviceFrames, build_stream, mutate, signed_votes, wide  # noqa: F401
from test_gpu_verify import gv, seeds_for  # noqa: F401  (gv: fixture)

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
KEYS = ("kind", "view", "seq", "dig", "rep", "sig")


def sign_votes(gv, n_keys, kind, view, seq, dig, rep):
    """The votes (kind, view, seq, dig)[i] signed by replica rep[i]; a dict like signed_votes'."""
    n = len(rep)
    kind, view, seq = (np.asarray(kind, np.uint8), np.asarray(view, np.uint64), np.asarray(seq, np.uint64))
    env = np.zeros((n, 85), np.uint8)
    env[:, :4] = np.frombuffer(b"PBFT", np.uint8)
    env[:, 4] = kind
    env[:, 5:13] = view.astype("<u8").view(np.uint8).reshape(n, 8)
    env[:, 13:21] = seq.astype("<u8").view(np.uint8).reshape(n, 8)
    env[:, 21:] = dig
    rep = np.asarray(rep, np.uint16)
    R, S, pub = gv.sign(seeds_for(n_keys, tag=1000 + n_keys), rep, env, 85)  # (signed_votes' key set)
    return dict(kind=kind, view=view, seq=seq, dig=np.asarray(dig, np.uint8), rep=rep,
                sig=np.concatenate([R, S], axis=1), pub=pub), env


class Case:
    """One network's stream: a mixed part (pooled envelopes, forged signatures, mutants, PrePrepares) followed by the
    canonical votes of two known envelopes, `full` with 2f + 1 distinct signers and `short` with 2f."""

    def __init__(self, gv, n_keys, n_mixed, n_pool):
        rng = np.random.default_rng(n_keys)
        self.n_keys, self.f = n_keys, (n_keys - 1) // 3
        pk, pv, ps = rng.choice(np.array([1, 2], np.uint8), n_pool), wide(rng, n_pool), wide(rng, n_pool)
        pd = rng.integers(0, 256, (n_pool, 64), dtype=np.uint8)
        pk[1], pv[1], ps[1], pd[1] = 3 - pk[0], pv[0], ps[0], pd[0]  # a Prepare and a Commit for one (v, n, d)
        j = rng.integers(0, n_pool, n_mixed)
        mixed, _ = sign_votes(gv, n_keys, pk[j], pv[j], ps[j], pd[j], rng.integers(0, n_keys, n_mixed))
        self.pub = mixed.pop("pub")
        w = signed_votes(gv, n_keys, n_mixed, seed=n_keys + 1, kinds=(0,))  # signed PrePrepares, every 29th frame
        pp = np.arange(n_mixed) % 29 == 7
        for k in KEYS:
            mixed[k][pp] = w[k][pp]
        assert (w["pub"] == self.pub).all()
        need = 2 * self.f + 1
        signers = rng.permutation(n_keys)
        dig = rng.integers(0, 256, (2, 64), dtype=np.uint8)
        rep = np.concatenate([signers[:need], signers[:need - 1]])
        which = np.repeat([0, 1], [need, need - 1])
        known, env = sign_votes(gv, n_keys, np.full(len(rep), 2), np.full(len(rep), 3), (2**40 + 1 + which), dig[which],
                                rep)
        known.pop("pub")
        self.full, self.short = env[0], env[-1]
        s1, o1, l1, _ = build_stream(mixed, n_keys, seed=n_keys)
        s2, o2, l2, canon = build_stream(known, n_keys, seed=1, canonical_only=True)
        assert canon.all()
        self.stream = np.concatenate([s1, s2])
        self.off = np.concatenate([o1, o2 + np.uint64(len(s1))])
        self.flen = np.concatenate([l1, l2])
        self.n = len(self.off)
        # the yardstick of the host form, computed once
        assert gv.set_keys(self.pub).all()
        self.bm, self.heads, self.records = gv.verify_frames(self.stream, self.off, self.flen)

    def reference(self, records, bits, env_cap):
        """(env_idx, envelopes, n_env, signers, counts) by the numpy references over `records` and `bits`."""
        from pbft_amd import group_reference, tally_reference
        key = records[:, 150:152].copy().view(np.uint16).reshape(-1)
        idx, envs, n_env = group_reference(records[:, 64:149], key == 0xFFFF, env_cap)
        sets, counts = tally_reference(bits, key, idx, env_cap, self.n_keys)
        return idx, envs, n_env, sets, counts

    def check_quorums(self, envs, counts):
        """The envelope with 2f + 1 valid distinct signers passes quorum(., 2f + 1); the one with 2f does not, and
        passes quorum(., 2f)."""
        from pbft_amd import quorum
        e_full = np.nonzero((envs == self.full).all(axis=1))[0]
        e_short = np.nonzero((envs == self.short).all(axis=1))[0]
        assert len(e_full) == 1 and len(e_short) == 1
        f = self.f
        assert counts[e_full[0]] == 2 * f + 1 and counts[e_short[0]] == 2 * f
        assert quorum(counts, 2 * f + 1)[e_full[0]] and not quorum(counts, 2 * f + 1)[e_short[0]]
        assert quorum(counts, 2 * f)[e_short[0]]


@pytest.fixture(scope="module")
def cases(gv):
    return {4: Case(gv, 4, 1990, 12), 256: Case(gv, 256, 1660, 24)}


class TallyOut:
    """The device form's grouping and tally outputs, poisoned, each followed by a poisoned guard."""
    FILL = dict(idx=0xA5, env=0x5A, cnt=0xC3, sets=0x3C, counts=0x96)

    def __init__(self, n, cap, n_keys):
        import torch
        self.n, self.cap, self.W = n, cap, (n_keys + 63) // 64
        self.size = dict(idx=4 * n, env=85 * cap, cnt=8, sets=8 * cap * self.W, counts=4 * cap)
        dev = torch.device("cuda", 0)
        self.t = {k: torch.full((self.size[k] + GUARD,), self.FILL[k], dtype=torch.uint8, device=dev) for k in self.size}

    def args(self):
        return dict(env_cap=self.cap, d_env_idx=self.t["idx"].data_ptr(), d_envelopes=self.t["env"].data_ptr(),
                    d_n_env=self.t["cnt"].data_ptr(), d_signers=self.t["sets"].data_ptr(),
                    d_count=self.t["counts"].data_ptr())

    def raw(self):
        return {k: v.cpu().numpy() for k, v in self.t.items()}

    def untouched(self):
        return all((a == self.FILL[k]).all() for k, a in self.raw().items())

    def read(self):
        r = self.raw()
        for k, a in r.items():
            assert (a[self.size[k]:] == self.FILL[k]).all(), ("guard overwritten", k)
        cut = {k: a[:self.size[k]].copy() for k, a in r.items()}
        return (cut["idx"].view(np.uint32), cut["env"].reshape(self.cap, 85), cut["cnt"].view(np.uint32),
                cut["sets"].view(np.uint64).reshape(self.cap, self.W), cut["counts"].view(np.uint32))


def same(got, exp, where):
    for g, e, name in zip(got, exp, ("env_idx", "envelopes", "n_env", "signers", "counts")):
        assert g.shape == e.shape and (g == e).all(), (where, name)


@pytest.mark.parametrize("n_keys", [4, 256])
def test_host_form(gv, cases, n_keys):
    from pbft_amd import bitmap_to_bool
    c = cases[n_keys]
    assert gv.set_keys(c.pub).all()
    bits = bitmap_to_bool(c.bm, c.n)
    st = c.heads["status"]
    assert set(st.tolist()) == {0, 1, 2, 3, 4, 5} and bits.sum() > c.n // 2 and (~bits & (st == 0)).sum() > 50
    assert ((st == 0) & (c.heads["kind"] == 0)).any()  # signed PrePrepares went through
    cap = 512  # (forged digests, flipped bits and PrePrepares are envelopes of their own: a few hundred)
    exp = c.reference(c.records, bits, cap)
    assert 2 < exp[2][0] <= cap and exp[2][1] == 0 and (exp[0][st != 0] == NONE).all()
    assert np.unique(exp[0][st == 0], return_counts=True)[1].max() > 20  # envelopes repeat
    bm, heads, idx, envs, n_env, sets, counts = gv.verify_frames_tally(c.stream, c.off, c.flen, cap)
    assert (bm == c.bm).all() and (heads == c.heads).all()
    same((idx, envs, n_env, sets, counts), exp, n_keys)
    c.check_quorums(envs, counts)
    # a Prepare and a Commit for one (view, seq, digest) are two envelopes
    k = min(int(n_env[0]), 60)  # (the pool's envelopes appear early)
    body = envs[:k, 5:]
    assert any((body[a] == body[b]).all() and envs[a, 4] != envs[b, 4] for a in range(k) for b in range(a + 1, k))
    # env_idx is optional
    got = gv.verify_frames_tally(c.stream, c.off, c.flen, cap, want_env_idx=False)
    assert got[2] is None and (got[0] == c.bm).all()
    same((exp[0],) + got[3:], exp, "no env_idx")


@pytest.mark.parametrize("n_keys", [4, 256])
def test_device_form(gv, cases, n_keys):
    import torch
    c = cases[n_keys]
    assert gv.set_keys(c.pub).all()
    ts = torch.cuda.Stream()
    ref = DeviceFrames(c.stream, c.off, c.flen)
    gv.verify_frames_device(d_bitmap=ref.bm.data_ptr(), stream=ts.cuda_stream, **ref.args(n_keys))
    ts.synchronize()
    r_rec, r_heads, r_bits = ref.read()
    cap = 512
    d, out = DeviceFrames(c.stream, c.off, c.flen), TallyOut(c.n, cap, n_keys)
    gv.verify_frames_tally_device(d_bitmap=d.bm.data_ptr(), stream=ts.cuda_stream, **d.args(n_keys), **out.args())
    ts.synchronize()
    rec, heads, bits = d.read()
    assert (d.bm.cpu().numpy() == ref.bm.cpu().numpy()).all()  # word for word, guard included
    assert (heads == r_heads).all() and (rec == r_rec).all()
    # ... and verify_frames' on every frame the device settled; the deferred ones are out of every envelope
    from pbft_amd import bitmap_to_bool
    settled = heads["status"] != EDEFER
    assert settled.sum() > c.n * 2 // 3 and (~settled).sum() > 50
    assert (heads[settled] == c.heads[settled]).all() and (rec[settled] == c.records[settled]).all()
    assert (bits[settled] == bitmap_to_bool(c.bm, c.n)[settled]).all() and not bits[~settled].any()
    got = out.read()
    exp = c.reference(rec, bits, cap)
    same(got, exp, n_keys)
    assert (got[0][~settled] == NONE).all()
    c.check_quorums(got[1], got[4])  # (the known votes are canonical: settled on the device)


def test_env_cap_below_the_distinct_count(gv, cases):
    """Host and device form with room for fewer envelopes than the stream has: later envelopes lose their votes (and
    are counted), the kept ones keep exactly theirs."""
    import torch
    from pbft_amd import bitmap_to_bool
    c = cases[4]
    assert gv.set_keys(c.pub).all()
    bits = bitmap_to_bool(c.bm, c.n)
    roomy = c.reference(c.records, bits, 512)
    cap = int(roomy[2][0]) - 3
    exp = c.reference(c.records, bits, cap)
    assert exp[2][0] == cap + 3 and exp[2][1] > 0 and (exp[3] == roomy[3][:cap]).all()
    bm, heads, idx, envs, n_env, sets, counts = gv.verify_frames_tally(c.stream, c.off, c.flen, cap)
    assert (bm == c.bm).all() and (heads == c.heads).all()
    same((idx, envs, n_env, sets, counts), exp, "host")
    d, out = DeviceFrames(c.stream, c.off, c.flen), TallyOut(c.n, 2, 4)
    ts = torch.cuda.Stream()
    gv.verify_frames_tally_device(d_bitmap=d.bm.data_ptr(), stream=ts.cuda_stream, **d.args(4), **out.args())
    ts.synchronize()
    rec, heads, bits = d.read()
    exp = c.reference(rec, bits, 2)
    assert exp[2][0] > 2 and exp[2][1] > 0
    same(out.read(), exp, "device")


def test_no_frames_and_argument_errors(gv, cases):
    import torch
    from pbft_amd import PbftError
    c = cases[4]
    assert gv.set_keys(c.pub).all()
    none64, none32 = np.zeros(0, np.uint64), np.zeros(0, np.uint32)
    bm, heads, idx, envs, n_env, sets, counts = gv.verify_frames_tally(b"", none64, none32, 5)
    assert len(bm) == 0 and len(heads) == 0 and len(idx) == 0
    assert n_env.tolist() == [0, 0] and envs.shape == (5, 85) and not envs.any() and not sets.any() and not counts.any()
    out = TallyOut(0, 5, 4)
    gv.verify_frames_tally_device(d_stream=0, stream_bytes=0, d_off=0, d_len=0, n_replicas=4, n=0, d_records=0,
                                  d_heads=0, d_bitmap=0, **out.args())
    torch.cuda.synchronize()
    idx, envs, n_env, sets, counts = out.read()
    assert n_env.tolist() == [0, 0] and not envs.any() and not sets.any() and not counts.any()
    # refused calls: env_cap = 0 with frames, null or misaligned outputs -- nothing is enqueued, nothing written
    with pytest.raises(PbftError) as e:
        gv.verify_frames_tally(c.stream, c.off, c.flen, 0)
    assert e.value.code == -1
    d, out = DeviceFrames(c.stream[:int(c.off[8])], c.off[:8], c.flen[:8]), TallyOut(8, 4, 4)
    good = {**d.args(4), **out.args(), "d_bitmap": d.bm.data_ptr()}
    for bad in (dict(env_cap=0), dict(d_env_idx=0), dict(d_envelopes=0), dict(d_n_env=0), dict(d_signers=0),
                dict(d_count=0), dict(d_bitmap=0), dict(d_env_idx=good["d_env_idx"] + 2),
                dict(d_signers=good["d_signers"] + 4), dict(d_count=good["d_count"] + 2), dict(n_replicas=0),
                dict(d_records=good["d_records"] + 8)):
        with pytest.raises(PbftError) as e:
            gv.verify_frames_tally_device(**{**good, **bad})
        assert e.value.code == -1, bad
    torch.cuda.synchronize()
    assert out.untouched()
    rec, hd, bmp = d.rec.cpu().numpy(), d.hd.cpu().numpy(), d.bm.cpu().numpy()
    assert (rec == 0xA5).all() and (hd == 0x5A).all() and (bmp == 0xC3).all()
