"""GPU vote tally (pbft_tally_device / pbft_verify_votes_tally) against tally_reference, exact equality:
synthetic rows without crypto (sizes around the wave and block edges, both orderings, both input layouts, out-of-range
indices with their bits set, duplicates, guarded outputs), accumulation over pieces, a signed adversarial round end to
end on one stream (device form, blocking host form, the host form's chunk schedule), and a hipGraph capture."""
import numpy as np
import pytest

from test_gpu_verify import adversarial, coracle, gv, oracle_bits, round_batch  # noqa: F401  (gv, coracle: fixtures)

pytestmark = pytest.mark.gpu
GUARD = 256  # poisoned bytes behind each output
ROW, ROW_KEY, ROW_ENV = 72, 64, 68  # PBFT_VOTES_ROW_BYTES, _KEY, _ENV


def dev_bytes(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(torch.device("cuda", 0))


def pack_bits(bits, fill_tail=False):
    """bool[n] -> LSB-first u64 words; fill_tail sets the bits past n in the last word (the device form takes any
    bitmap: rows past N must not count whatever those bits say)."""
    n = len(bits)
    b = np.zeros((n + 63) // 64 * 64, dtype=bool)
    b[:n] = bits
    if fill_tail:
        b[n:] = True
    return np.packbits(b, bitorder="little").view(np.uint64)


class Outputs:
    """d_signers [n_env][W] u64 and d_count [n_env] u32, poisoned, each followed by a poisoned guard."""

    def __init__(self, n_env, n_signers):
        import torch
        self.n_env, self.W = n_env, (n_signers + 63) // 64
        dev = torch.device("cuda", 0)
        self.s = torch.full((n_env * self.W * 8 + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.c = torch.full((n_env * 4 + GUARD,), 0x5A, dtype=torch.uint8, device=dev)

    def read(self):
        s, c = self.s.cpu().numpy(), self.c.cpu().numpy()
        ns, nc = self.n_env * self.W * 8, self.n_env * 4
        assert (s[ns:] == 0xA5).all() and (c[nc:] == 0x5A).all(), "guard region overwritten"
        return s[:ns].view(np.uint64).reshape(self.n_env, self.W).copy(), c[:nc].view(np.uint32).copy()


def run_tally(gv, bits, key_idx, env_idx, n_env, n_signers, layout="columns", out=None, flags=0, lo=0, hi=None,
              fill_tail=True):
    """Tally rows [lo, hi) (lo a multiple of 64) on a torch stream; returns the Outputs."""
    import torch
    hi = len(bits) if hi is None else hi
    n = hi - lo
    ts = torch.cuda.Stream()
    with torch.cuda.stream(ts):
        out = out or Outputs(n_env, n_signers)
        dB = dev_bytes(pack_bits(bits[lo:hi], fill_tail))
        if layout == "columns":
            dK, dE = dev_bytes(key_idx[lo:hi].astype(np.uint16)), dev_bytes(env_idx[lo:hi].astype(np.uint32))
            pk, pe, sk, se = dK.data_ptr(), dE.data_ptr(), 2, 4
        else:  # the 72-byte votes rows: signature bytes (noise here), key_idx at 64, two zero bytes, env_idx at 68
            rows = np.random.default_rng(n).integers(0, 256, (n, ROW), dtype=np.uint8)
            rows[:, ROW_KEY:ROW_KEY + 4] = key_idx[lo:hi].astype(np.uint32).view(np.uint8).reshape(n, 4)
            rows[:, ROW_ENV:ROW_ENV + 4] = env_idx[lo:hi].astype(np.uint32).view(np.uint8).reshape(n, 4)
            dK = dE = dev_bytes(rows)
            pk, pe, sk, se = dK.data_ptr() + ROW_KEY, dK.data_ptr() + ROW_ENV, ROW, ROW
        gv.tally_device(dB.data_ptr(), pk, pe, n, n_env, n_signers, out.s.data_ptr(), out.c.data_ptr(),
                        ts.cuda_stream, key_stride=sk, env_stride=se, flags=flags)
    ts.synchronize()
    return out


def synthetic(rng, n, n_env, n_signers, order):
    """Rows of a round: ~85 % valid bits, duplicated (signer, envelope) pairs, ~1 % of rows with env_idx >= n_env and
    ~1 % with key_idx >= n_signers (at least one each from 8 rows up), bits set on both groups."""
    key_idx = rng.integers(0, n_signers, n).astype(np.uint16)
    env_idx = rng.integers(0, n_env, n).astype(np.uint32)
    bits = rng.random(n) < 0.85
    if n >= 8:
        d = max(1, n // 16)  # duplicates of valid rows
        src, dst = rng.integers(0, n, d), rng.integers(0, n, d)
        key_idx[dst], env_idx[dst] = key_idx[src], env_idx[src]
        bits[src] = bits[dst] = True
        m = max(1, n // 100)
        bad_e, bad_k = rng.choice(n, 2 * m, replace=False).reshape(2, m)
        env_idx[bad_e] = rng.choice(np.array([n_env, n_env + 1, 2**31, 2**32 - 1], dtype=np.uint32), m)
        key_idx[bad_k] = rng.choice(np.array([n_signers, n_signers + 63, 65535], dtype=np.uint16), m)
        bits[bad_e] = bits[bad_k] = True
    if order == "sorted":  # the replica's layout: an envelope's votes contiguous, signers ascending
        p = np.lexsort((key_idx, env_idx))
    else:
        p = rng.permutation(n)
    return bits[p], key_idx[p], env_idx[p]


SIZES = [1, 63, 64, 65, 4097, 65536 + 77]


@pytest.mark.parametrize("n_signers,n_env", [(1, 1), (4, 3), (64, 16), (65, 16), (256, 512), (1000, 7)])
def test_synthetic_rows_match_reference(gv, n_signers, n_env):
    from pbft_amd import tally_reference
    rng = np.random.default_rng(100 * n_signers + n_env)
    for n in SIZES:
        for order in ("sorted", "permuted"):
            bits, key_idx, env_idx = synthetic(rng, n, n_env, n_signers, order)
            exp_s, exp_c = tally_reference(bits, key_idx, env_idx, n_env, n_signers)
            for layout in ("columns", "rows"):
                got_s, got_c = run_tally(gv, bits, key_idx, env_idx, n_env, n_signers, layout).read()
                where = (n, order, layout)
                assert (got_s == exp_s).all(), where
                assert (got_c == exp_c).all(), where


def test_argument_checks(gv):
    from pbft_amd import PbftError
    n, n_env, n_signers = 128, 4, 64
    rng = np.random.default_rng(5)
    bits, key_idx, env_idx = synthetic(rng, n, n_env, n_signers, "sorted")
    out = Outputs(n_env, n_signers)
    dB, dK, dE = dev_bytes(pack_bits(bits)), dev_bytes(key_idx), dev_bytes(env_idx)
    good = dict(d_bitmap=dB.data_ptr(), d_key_idx=dK.data_ptr(), d_env_idx=dE.data_ptr(), n=n, n_env=n_env,
                n_signers=n_signers, d_signers=out.s.data_ptr(), d_count=out.c.data_ptr())
    for bad in (dict(n_signers=0), dict(n_signers=65536), dict(key_stride=1), dict(key_stride=3), dict(key_stride=0),
                dict(env_stride=2), dict(env_stride=6), dict(env_stride=0), dict(flags=2), dict(flags=3),
                dict(d_bitmap=0), dict(d_key_idx=0), dict(d_env_idx=0), dict(d_signers=0), dict(d_count=0),
                dict(d_signers=0, n=0)):
        with pytest.raises(PbftError) as e:
            gv.tally_device(**{**good, **bad})
        assert e.value.code == -1, bad
    # n_env = 0 writes nothing; N = 0 zeroes the sets and the counts
    import torch
    gv.tally_device(**{**good, "n_env": 0})
    torch.cuda.synchronize()
    s, c = out.read()
    assert (s == 0xA5A5A5A5A5A5A5A5).all() and (c == 0x5A5A5A5A).all()
    gv.tally_device(**{**good, "n": 0, "d_bitmap": 0, "d_key_idx": 0, "d_env_idx": 0})
    torch.cuda.synchronize()
    s, c = out.read()
    assert not s.any() and not c.any()


@pytest.mark.parametrize("layout", ["columns", "rows"])
def test_accumulate_over_pieces(gv, layout):
    from pbft_amd import TALLY_ACCUMULATE, tally_reference
    n, n_env, n_signers, m = 4097 + 640, 40, 130, 1984  # m: a multiple of 64 that is no multiple of the block
    rng = np.random.default_rng(77)
    bits, key_idx, env_idx = synthetic(rng, n, n_env, n_signers, "permuted")
    exp_s, exp_c = tally_reference(bits, key_idx, env_idx, n_env, n_signers)
    # the first piece without the flag overwrites the poison, the second one ORs into it
    out = run_tally(gv, bits, key_idx, env_idx, n_env, n_signers, layout, lo=0, hi=m, fill_tail=False)
    s1, c1 = out.read()
    p_s, p_c = tally_reference(bits[:m], key_idx[:m], env_idx[:m], n_env, n_signers)
    assert (s1 == p_s).all() and (c1 == p_c).all()
    run_tally(gv, bits, key_idx, env_idx, n_env, n_signers, layout, out=out, flags=TALLY_ACCUMULATE, lo=m)
    s2, c2 = out.read()
    assert (s2 == exp_s).all() and (c2 == exp_c).all()
    # the same piece again changes nothing (OR is idempotent); an empty accumulating call only recounts
    run_tally(gv, bits, key_idx, env_idx, n_env, n_signers, layout, out=out, flags=TALLY_ACCUMULATE, lo=m)
    s3, c3 = out.read()
    assert (s3 == exp_s).all() and (c3 == exp_c).all()
    # without the flag the stale sets are overwritten
    run_tally(gv, bits, key_idx, env_idx, n_env, n_signers, layout, out=out, lo=m)
    s4, c4 = out.read()
    q_s, q_c = tally_reference(bits[m:], key_idx[m:], env_idx[m:], n_env, n_signers)
    assert (s4 == q_s).all() and (c4 == q_c).all()


@pytest.fixture(scope="module")
def signed_round(gv, coracle):
    """64 keys x 8 seqs x {Prepare, Commit} = 1,024 GPU-signed votes, mutated across the adversarial classes; then a
    valid vote duplicated under its envelope, and a vote moved to another signer whose own vote is spoiled (so the
    envelope loses both).  Returns the rows, the envelope table and the C oracle's bits."""
    seeds, pub, R, S, key_idx, msg = round_batch(gv, 64, 8, tag=53)
    rng = np.random.default_rng(53)
    R, S, K, M, idx = adversarial(rng, pub, R, S, key_idx, msg)
    touched = set(int(i) // 64 for i in idx)
    intact = [b for b in range(16) if b not in touched]  # (kind, seq) blocks of 64 rows no mutation fell into
    assert len(intact) >= 4
    b_dup, b_mov = intact[0], intact[1]
    a = 64 * b_dup + 9  # the duplicated vote (appended)
    mv = 64 * b_mov + 20  # the moved vote: signer 20's signature claimed for signer 41 ...
    K[mv] = 41
    S[64 * b_mov + 41, 0] ^= 1  # ... whose own vote does not verify
    R, S, K, M = (np.concatenate([x, x[a:a + 1]]) for x in (R, S, K, M))
    env, inv = np.unique(M, axis=0, return_inverse=True)
    ei = inv.reshape(-1).astype(np.uint32)
    exp = oracle_bits(coracle, pub, R, S, K, M, 85)
    return dict(pub=pub, R=R, S=S, K=K, ei=ei, env=env, M=M, exp=exp, intact=intact[2:], b_dup=b_dup, b_mov=b_mov)


def device_round(gv, r, n_env, ts):
    """The round's device columns + outputs, and a closure that enqueues verify_votes_device then tally_device."""
    import torch
    n = len(r["R"])
    with torch.cuda.stream(ts):
        envp = np.zeros(n_env * 85 + 64, np.uint8)
        envp[: n_env * 85] = r["env"].reshape(-1)
        d = dict(R=dev_bytes(r["R"]), S=dev_bytes(r["S"]), K=dev_bytes(r["K"].astype(np.uint16)),
                 I=dev_bytes(r["ei"]), E=dev_bytes(envp),
                 B=torch.zeros((n + 63) // 64, dtype=torch.int64, device=torch.device("cuda", 0)))
        out = Outputs(n_env, 64)

    def enqueue(stream):
        gv.verify_votes_device(d["R"].data_ptr(), d["S"].data_ptr(), d["K"].data_ptr(), d["I"].data_ptr(),
                               d["E"].data_ptr(), n_env, n, d["B"].data_ptr(), stream)
        gv.tally_device(d["B"].data_ptr(), d["K"].data_ptr(), d["I"].data_ptr(), n, n_env, 64, out.s.data_ptr(),
                        out.c.data_ptr(), stream)
    return d, out, enqueue


def test_signed_round_end_to_end(gv, signed_round):
    import torch
    from pbft_amd import bitmap_to_bool, quorum, tally_reference
    r = signed_round
    n, n_env = len(r["R"]), len(r["env"])
    assert gv.set_keys(r["pub"]).all()
    exp_s, exp_c = tally_reference(r["exp"], r["K"], r["ei"], n_env, 64)
    ts = torch.cuda.Stream()
    d, out, enqueue = device_round(gv, r, n_env, ts)
    enqueue(ts.cuda_stream)
    ts.synchronize()
    got_s, got_c = out.read()
    assert (bitmap_to_bool(d["B"].cpu().numpy().view(np.uint64), n) == r["exp"]).all()
    assert (got_s == exp_s).all() and (got_c == exp_c).all()
    # an envelope whose 64 signers are all intact has them all, the duplicated vote included once
    first = r["ei"][::64][:16]  # block b's envelope (row 64 b is mutated in no intact block)
    for b in r["intact"] + [r["b_dup"]]:
        assert got_c[first[b]] == 64 and got_s[first[b], 0] == 2**64 - 1
    # the moved vote counts for neither signer
    e = first[r["b_mov"]]
    assert got_c[e] == 62 and got_s[e, 0] == (2**64 - 1) ^ (1 << 20) ^ (1 << 41)
    assert quorum(got_c, 43).sum() == (exp_c >= 43).sum() >= 14
    # blocking host form: the same three arrays, the bitmap of verify_votes
    bm, hs, hc = gv.verify_votes_tally(r["R"], r["S"], r["K"], r["ei"], r["env"])
    assert (bm == gv.verify_votes(r["R"], r["S"], r["K"], r["ei"], r["env"])).all()
    assert (bitmap_to_bool(bm, n) == r["exp"]).all()
    assert (hs == exp_s).all() and (hc == exp_c).all()


def chunk_end(lo, n, F=1 << 16, C=1 << 18):
    """pbft_votes_chunk_end (include/pbft_verify.h): the host votes forms' chunk schedule."""
    r = n - lo
    if n <= C or lo >= n:
        return n
    if lo == 0:
        return F
    if lo == F:
        return min(3 * F, n)
    if r > C + 3 * F:
        return lo + C
    if r > 4 * F:
        return lo + ((r - 3 * F) & ~63)
    if r > 2 * F:
        return lo + ((r - F) & ~63)
    return n


@pytest.mark.parametrize("memory", ["pageable", "pinned"])
def test_host_form_crosses_chunk_schedule(gv, signed_round, memory):
    """N = 2^18 + 64 * 3 + 5 rows tiled from the round: the host form runs three chunks on two streams, each tallied
    behind its own kernels into one set.  Pageable columns travel as 72-byte rows through the context's staging,
    pinned ones are copied as columns: the tally reads the chunk's key and envelope indices in either layout."""
    import torch
    from pbft_amd import bitmap_to_bool, tally_reference
    r = signed_round
    n0, n_env = len(r["R"]), len(r["env"])
    N = (1 << 18) + 64 * 3 + 5
    assert gv.set_keys(r["pub"]).all()
    t = np.arange(N) % n0
    R, S, K, ei = r["R"][t], r["S"][t], r["K"][t], r["ei"][t]
    # signer k's votes stay valid in chunk k % 3 of the schedule alone (spoiled elsewhere), so a set is complete only
    # if every chunk was tallied
    ends, lo = [], 0
    while lo < N:
        lo = chunk_end(lo, N)
        ends.append(lo)
    assert len(ends) == 3
    spoil = (K % 3) != np.searchsorted(np.array(ends), np.arange(N), side="right")
    S[spoil] = 0  # (s = 0 verifies under no key, whatever the row held before)
    exp = r["exp"][t] & ~spoil
    E = r["env"]
    if memory == "pinned":
        R, S, K, ei, E = (torch.from_numpy(np.ascontiguousarray(a)).pin_memory().numpy() for a in (R, S, K, ei, E))
    bm, hs, hc = gv.verify_votes_tally(R, S, K, ei, E)
    assert (bm == gv.verify_votes(R, S, K, ei, E)).all()
    got = bitmap_to_bool(bm, N)
    assert (got == exp).all(), np.nonzero(got != exp)[0][:8]
    exp_s, exp_c = tally_reference(exp, K, ei, n_env, 64)
    assert (hs == exp_s).all() and (hc == exp_c).all()
    first = r["ei"][::64][:16]
    for b in r["intact"] + [r["b_dup"]]:
        assert hc[first[b]] == 64


def test_verify_and_tally_captured_in_one_graph(gv, coracle, signed_round):
    """reserve + one warm call, then verify_votes_device + tally_device captured as one linear chain on one stream and
    replayed twice with different inputs in the same buffers."""
    import torch
    from pbft_amd import bitmap_to_bool, tally_reference
    r = signed_round
    n, n_env = len(r["R"]), len(r["env"])
    assert gv.set_keys(r["pub"]).all()
    gv.reserve(n)
    ts = torch.cuda.Stream()
    d, out, enqueue = device_round(gv, r, n_env, ts)
    enqueue(ts.cuda_stream)  # warm: the envelope-schedule buffer grows outside the capture
    ts.synchronize()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        enqueue(torch.cuda.current_stream().cuda_stream)
    S2 = r["S"].copy()
    S2[100:700:3, 5] ^= 0x10
    exp2 = oracle_bits(coracle, r["pub"], r["R"], S2, r["K"], r["M"], 85)
    assert exp2.sum() < r["exp"].sum()
    for rep, (S, exp) in enumerate(((r["S"], r["exp"]), (S2, exp2))):
        d["S"].copy_(dev_bytes(S))
        d["B"].fill_(-1)  # stale bitmap words: a tally that ran ahead of the verify would count them
        out.s.fill_(0xA5)
        out.c.fill_(0x5A)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got_s, got_c = out.read()
        assert (bitmap_to_bool(d["B"].cpu().numpy().view(np.uint64), n) == exp).all(), rep
        exp_s, exp_c = tally_reference(exp, r["K"], r["ei"], n_env, 64)
        bad = np.nonzero((got_s != exp_s).any(axis=1) | (got_c != exp_c))[0]
        assert not len(bad), (rep, bad[:4], got_s[bad[:4], 0], exp_s[bad[:4], 0])
