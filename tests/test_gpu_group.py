"""GPU envelope grouping (pbft_group_envelopes_device) against group_reference, exact equality: sizes around the wave,
block and scan-word edges; all-equal, all-distinct and skewed batches in runs and permuted; keys that differ in one
byte; both input layouts (an 85-byte column at every alignment, 160-byte records in place) with and without the skip
column; overflow; truncated hashes (long probe chains) under several seeds; a hipGraph capture; argument errors.
Every output has poisoned guard bytes behind it, checked intact."""
import numpy as np
import pytest

from test_gpu_frames import GUARD
from test_gpu_verify import gv  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
SIZES = [1, 63, 64, 65, 4097]


def dev_bytes(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(torch.device("cuda", 0))


def pool(rng, m):
    """m distinct envelopes: "PBFT", kind, view, seq, random digest."""
    e = rng.integers(0, 256, (m, 85), dtype=np.uint8)
    e[:, :4] = np.frombuffer(b"PBFT", np.uint8)
    e[:, 4] = rng.integers(1, 3, m)
    e[:, 13:21] = np.arange(m, dtype="<u8").view(np.uint8).reshape(m, 8)  # (distinct whatever the digests are)
    return e


def batches(rng, n):
    """(name, rows (n, 85)) of the shapes a batch can take."""
    p = pool(rng, max(n, 40))
    yield "equal", np.repeat(p[:1], n, axis=0)
    yield "distinct", p[rng.permutation(len(p))[:n]]
    # ~40 envelopes, skewed: envelope j about twice as frequent as envelope j + 4; in runs of 256 rows, then permuted
    w = 0.5 ** (np.arange(40) / 4.0)
    pick = rng.choice(40, n, p=w / w.sum())
    runs = np.repeat(rng.choice(40, (n + 255) // 256, p=w / w.sum()), 256)[:n]
    yield "runs", p[runs]
    yield "permuted", p[pick]


class Outputs:
    """d_env_idx [n] u32, d_envelopes [env_cap][85], d_n_env [2] u32: poisoned, each followed by a poisoned guard."""

    def __init__(self, n, env_cap):
        import torch
        dev = torch.device("cuda", 0)
        self.n, self.cap = n, env_cap
        self.idx = torch.full((n * 4 + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.env = torch.full((env_cap * 85 + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
        self.cnt = torch.full((8 + GUARD,), 0xC3, dtype=torch.uint8, device=dev)

    def poison(self):
        self.idx.fill_(0xA5)
        self.env.fill_(0x5A)
        self.cnt.fill_(0xC3)

    def untouched(self):
        idx, env, cnt = self.idx.cpu().numpy(), self.env.cpu().numpy(), self.cnt.cpu().numpy()
        return (idx == 0xA5).all() and (env == 0x5A).all() and (cnt == 0xC3).all()

    def read(self):
        idx, env, cnt = self.idx.cpu().numpy(), self.env.cpu().numpy(), self.cnt.cpu().numpy()
        ni, ne = self.n * 4, self.cap * 85
        assert (idx[ni:] == 0xA5).all() and (env[ne:] == 0x5A).all() and (cnt[8:] == 0xC3).all(), "guard overwritten"
        return (idx[:ni].copy().view(np.uint32), env[:ne].reshape(self.cap, 85).copy(), cnt[:8].copy().view(np.uint32))


class Inputs:
    """The rows on the device as an 85-byte column starting `shift` bytes into its buffer (the buffer ends with the
    last row's last byte), or as 160-byte records; with a key column (u16, 0xFFFF = skipped) or without."""

    def __init__(self, rows, skip, layout, shift=0):
        n = len(rows)
        key = np.arange(n, dtype=np.uint16) % 251
        if skip is not None:
            key[skip] = 0xFFFF
        if layout == "records":
            rec = np.random.default_rng(n).integers(0, 256, (n, 160), dtype=np.uint8)
            rec[:, 64:149] = rows
            rec[:, 150:152] = key.view(np.uint8).reshape(n, 2)
            self.buf = dev_bytes(rec)
            self.msg, self.stride = self.buf.data_ptr() + 64, 160
            self.key, self.key_stride = (self.buf.data_ptr() + 150, 160) if skip is not None else (0, 2)
        else:
            self.buf = dev_bytes(np.concatenate([np.full(shift, 0xEE, np.uint8), rows.reshape(-1)]))
            self.msg, self.stride = self.buf.data_ptr() + shift, 85
            self.kbuf = dev_bytes(key) if skip is not None else None
            self.key, self.key_stride = (self.kbuf.data_ptr() if skip is not None else 0), 2

    def args(self, n, env_cap, out):
        return dict(d_msg=self.msg, n=n, env_cap=env_cap, d_env_idx=out.idx.data_ptr(), d_envelopes=out.env.data_ptr(),
                    d_n_env=out.cnt.data_ptr(), msg_stride=self.stride, d_key_idx=self.key, key_stride=self.key_stride)


def run_group(gv, rows, skip, env_cap, layout="column", shift=0):
    import torch
    n = len(rows)
    ts = torch.cuda.Stream()
    with torch.cuda.stream(ts):
        inp, out = Inputs(rows, skip, layout, shift), Outputs(n, env_cap)
        gv.group_envelopes_device(stream=ts.cuda_stream, **inp.args(n, env_cap, out))
    ts.synchronize()
    return out.read()


def check(got, exp, where):
    for g, e, name in zip(got, exp, ("env_idx", "envelopes", "n_env")):
        assert g.shape == e.shape and (g == e).all(), (where, name, np.nonzero(np.atleast_1d(g != e).reshape(-1))[0][:8])


def skipped(rng, n):
    """~15 % of the rows, row 0 among them."""
    s = rng.random(n) < 0.15
    s[0] = True
    return s


@pytest.mark.parametrize("n", SIZES)
def test_batches_match_reference(gv, n):
    """Every shape at every size, in both layouts, with and without skipped rows; the column starts at byte n % 4 of
    its buffer, so with the odd stride every alignment of a row occurs."""
    from pbft_amd import group_reference
    rng = np.random.default_rng(n)
    for name, rows in batches(rng, n):
        for skip in (None, skipped(rng, n)):
            exp = group_reference(rows, skip, n)
            if skip is None:
                assert exp[2][0] == {"equal": 1, "distinct": n}.get(name, exp[2][0])
            for layout in ("column", "records"):
                got = run_group(gv, rows, skip, n, layout, shift=n % 4)
                check(got, exp, (n, name, skip is not None, layout))


def test_near_equal_keys(gv):
    """Pairs of envelopes that differ only in byte 4 (kind), only in byte 21 (the digest's first byte) or only in byte
    84 (the last byte) get different indices; so do triples that differ from a base in one bit of any byte."""
    from pbft_amd import group_reference
    rng = np.random.default_rng(84)
    base = pool(rng, 30)
    variants = [base]
    for byte in (4, 21, 84):
        v = base[1:].copy()
        v[:, byte] ^= 1
        variants.append(v)
    every = np.repeat(base[:1], 85 * 8, axis=0)  # base[0] with each single bit flipped
    every[np.arange(85 * 8), np.arange(85 * 8) // 8] ^= (1 << (np.arange(85 * 8) % 8)).astype(np.uint8)
    distinct = np.concatenate(variants + [every])
    rows = np.concatenate([distinct, distinct[rng.integers(0, len(distinct), 2200)]])[rng.permutation(len(distinct) + 2200)]
    exp = group_reference(rows, None, len(distinct))
    assert exp[2][0] == len(distinct) == 30 + 3 * 29 + 680
    for layout in ("column", "records"):
        check(run_group(gv, rows, None, len(distinct), layout), exp, layout)
    pair = np.stack([base[1], variants[3][0]] * 40)  # one wave, two envelopes that differ in byte 84 alone
    check(run_group(gv, pair, None, 4), group_reference(pair, None, 4), "byte 84")


@pytest.mark.parametrize("layout", ["column", "records"])
def test_overflow(gv, layout):
    """env_cap one below the distinct count, and env_cap = 1: the indices kept, the 0xFFFFFFFF rows, both n_env words;
    env_cap above the count: the table's tail is zeroed."""
    from pbft_amd import group_reference
    rng = np.random.default_rng(17)
    n = 1500
    rows = pool(rng, 40)[rng.integers(0, 40, n)]
    skip = skipped(rng, n)
    full = group_reference(rows, skip, 64)
    m = int(full[2][0])
    assert m == 40 and not full[1][m:].any()
    check(run_group(gv, rows, skip, 64, layout), full, "roomy")
    for cap in (m - 1, 1):
        exp = group_reference(rows, skip, cap)
        assert exp[2][0] == m and exp[2][1] == (full[0][~skip] >= cap).sum() > 0
        assert ((exp[0] == NONE) == (skip | (full[0] >= cap))).all()
        check(run_group(gv, rows, skip, cap, layout), exp, cap)


def test_long_chains_and_seeds(gv):
    """PBFT_OPT_GROUP_HASH_BITS 0 and 3 at 300 rows of 40 envelopes: every row down one probe chain, or down eight.
    Three seeds give the same output as the reference."""
    from pbft_amd import group_reference
    rng = np.random.default_rng(300)
    rows = pool(rng, 40)[rng.integers(0, 40, 300)]
    skip = skipped(rng, 300)
    exp = group_reference(rows, skip, 40)
    assert exp[2][0] == 40
    try:
        for bits in (0, 3, 64):
            gv.set_option(gv.OPT_GROUP_HASH_BITS, bits)
            for seed in (0, 0x0123456789ABCDEF, 2**64 - 1):
                gv.set_option(gv.OPT_GROUP_SEED, seed)
                check(run_group(gv, rows, skip, 40, "records"), exp, (bits, seed))
    finally:
        gv.set_option(gv.OPT_GROUP_HASH_BITS, 64)
    from pbft_amd import PbftError
    with pytest.raises(PbftError) as e:
        gv.set_option(gv.OPT_GROUP_HASH_BITS, 65)
    assert e.value.code == -1


def test_group_capture(gv):
    """group_reserve, then the call captured into a graph and replayed three times with the rows rewritten in the same
    buffer between replays: each replay is exact."""
    import torch
    from pbft_amd import group_reference
    rng = np.random.default_rng(5)
    n, cap = 1000, 48
    p = pool(rng, 60)
    inputs = [p[rng.integers(0, 40, n)], np.repeat(p[41:42], n, axis=0), p[rng.integers(0, 60, n)]]
    skips = [skipped(rng, n) for _ in inputs]
    gv.group_reserve(n)
    inp, out = Inputs(inputs[2], skips[2], "records"), Outputs(n, cap)
    gv.group_envelopes_device(**inp.args(n, cap, out))  # (an eager call first: the kernels are loaded)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gv.group_envelopes_device(stream=torch.cuda.current_stream().cuda_stream, **inp.args(n, cap, out))
    for rep, (rows, skip) in enumerate(zip(inputs, skips)):
        inp.buf.copy_(Inputs(rows, skip, "records").buf)
        out.poison()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        exp = group_reference(rows, skip, cap)
        check(out.read(), exp, rep)
    assert group_reference(inputs[2], skips[2], cap)[2][1] > 0  # the last replay overflowed


def test_argument_errors_write_nothing(gv):
    import torch
    from pbft_amd import PbftError
    rng = np.random.default_rng(2)
    n, cap = 128, 8
    rows = pool(rng, 8)[rng.integers(0, 8, n)]
    inp, out = Inputs(rows, skipped(rng, n), "records"), Outputs(n, cap)
    good = inp.args(n, cap, out)
    for bad in (dict(d_msg=0), dict(d_env_idx=0), dict(d_envelopes=0), dict(d_n_env=0),
                dict(d_env_idx=good["d_env_idx"] + 2), dict(d_n_env=good["d_n_env"] + 1),
                dict(d_key_idx=good["d_key_idx"] + 1), dict(msg_stride=84), dict(msg_stride=0), dict(key_stride=0),
                dict(key_stride=1), dict(key_stride=161), dict(env_cap=0), dict(n=2**31 + 1)):
        with pytest.raises(PbftError) as e:
            gv.group_envelopes_device(**{**good, **bad})
        assert e.value.code == -1, bad
    with pytest.raises(PbftError) as e:
        gv.group_reserve(2**31 + 1)
    assert e.value.code == -1
    torch.cuda.synchronize()
    assert out.untouched()
    # N = 0: n_env = {0, 0}, the table zeroed, nothing else written
    gv.group_envelopes_device(**{**good, "n": 0, "d_msg": 0, "d_env_idx": 0, "d_key_idx": 0})
    torch.cuda.synchronize()
    idx, env, cnt = out.read()
    assert (idx == 0xA5A5A5A5).all() and not env.any() and cnt.tolist() == [0, 0]
