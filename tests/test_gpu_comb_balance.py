"""PBFT_OPT_COMB_BALANCE: the 4-wave chain-form comb whose waves lower their issue priority as they progress.

The option changes only the order in which a SIMD issues its waves' instructions, so every bitmap must equal, bit for
bit, the bitmap of the same context with the option off and the C oracle's (oracle/liboracle.so).  The pair comb and
the paired-priority 8-wave form are forced off so that the 4-wave chain form runs from 2^16 signatures.  Each batch
holds 1 % adversarial lanes (flipped s, s + L, flipped R, a key index past the key set, ...: test_gpu_verify's
adversarial()).  64 keys: a wave of 64 lanes signs one envelope (the hash's wave-uniform schedule), and the shuffled
case mixes envelopes in every wave (its per-lane schedule).  The golden corpus runs once through the forced form,
tiled to the chain form's sizes.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT, golden_batches
from test_gpu_verify import adversarial, oracle_bits, round_batch, verify

pytestmark = pytest.mark.gpu

# exact multiple of the block; a last wave with one live lane; a partial last block and a partial wave; the first
# size past the paired-priority form's automatic range
SIZES = (65536, 65536 + 1, 65536 + 64 * 3 + 5, 131072 + 64)


@pytest.fixture(scope="module")
def gv():
    from pbft_amd import GpuBatchVerifier
    v = GpuBatchVerifier(0)
    yield v
    v.close()


@pytest.fixture(scope="module")
def coracle():
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))
    vp = ctypes.c_void_p
    lib.oracle_verify_batch.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32,
                                        ctypes.c_uint64, vp, ctypes.c_int]
    return lib


@pytest.fixture(scope="module")
def batch(gv, coracle):
    """131,328 signatures of 64 keys with 1 % adversarial lanes, and the oracle's bits (computed once)."""
    seeds, pub, R, S, key_idx, msg = round_batch(gv, 64, 1026, tag=18)
    assert gv.set_keys(pub).all()
    rng = np.random.default_rng(18)
    R2, S2, K2, M2, idx = adversarial(rng, pub, R, S, key_idx, msg)
    exp = oracle_bits(coracle, pub, R2, S2, K2, M2, 85)
    assert not exp[idx].any() and exp.sum() == len(R) - len(idx)
    assert (K2 >= len(pub)).any()  # a key index past the key set is among them
    for a in (R2, S2, K2, M2, exp):
        a.setflags(write=False)
    return pub, R2, S2, K2, M2, exp


@pytest.fixture()
def chain4(gv):
    """The 4-wave chain form at every size from 2^16: pair comb and paired-priority form off."""
    gv.set_option(gv.OPT_COMB_PAIR, 0)
    gv.set_option(gv.OPT_COMB_PRIO, 0)
    yield gv
    gv.set_option(gv.OPT_COMB_PAIR, 2)
    gv.set_option(gv.OPT_COMB_PRIO, 2)
    gv.set_option(gv.OPT_COMB_BALANCE, 2)


@pytest.mark.parametrize("n", SIZES)
def test_balance_on_off_and_oracle(chain4, batch, n):
    gv = chain4
    pub, R, S, K, M, exp = batch
    bms = {}
    for mode in (1, 0, 2):  # on, off, by batch size
        gv.set_option(gv.OPT_COMB_BALANCE, mode)
        got, bm = verify(gv, R[:n], S[:n], K[:n], M[:n], 85)
        assert (got == exp[:n]).all(), (n, mode, np.nonzero(got != exp[:n])[0][:10])
        if n % 64:
            assert int(bm[-1]) >> (n % 64) == 0  # bits past N are zero
        bms[mode] = bm
    assert (bms[1] == bms[0]).all() and (bms[2] == bms[0]).all()


def test_balance_shuffled_rows(chain4, batch):
    """Rows in random order: every wave mixes envelopes and keys (the hash's per-lane schedule runs)."""
    gv = chain4
    pub, R, S, K, M, exp = batch
    n = 65536 + 64 * 3 + 5
    perm = np.random.default_rng(181).permutation(len(R))[:n]
    for mode in (1, 0):
        gv.set_option(gv.OPT_COMB_BALANCE, mode)
        got, _ = verify(gv, R[perm], S[perm], K[perm], M[perm], 85)
        assert (got == exp[perm]).all(), (mode, np.nonzero(got != exp[perm])[0][:10])


def test_balance_votes_form(chain4, batch):
    """The votes form (an envelope table and an index per signature) with one envelope index past the table."""
    gv = chain4
    pub, R, S, K, M, exp = batch
    n = 65536 + 64 * 3 + 5
    env, inv = np.unique(M[:n], axis=0, return_inverse=True)
    env_idx = inv.reshape(-1).astype(np.uint32)
    bad = 40_000 + int(np.argmax(exp[40_000:n]))  # an accepted lane
    env_idx[bad] = len(env) + 7
    want = exp[:n].copy()
    want[bad] = False
    from pbft_amd import bitmap_to_bool
    for mode in (1, 0):
        gv.set_option(gv.OPT_COMB_BALANCE, mode)
        got = bitmap_to_bool(gv.verify_votes(R[:n], S[:n], K[:n], env_idx, env), n)
        assert (got == want).all(), (mode, np.nonzero(got != want)[0][:10])


def test_balance_captured_replay(chain4, batch):
    """One forced launch captured into a HIP graph and replayed twice over a bitmap pre-filled with ones."""
    import torch
    from pbft_amd import bitmap_to_bool
    gv = chain4
    pub, R, S, K, M, exp = batch
    n = 65536 + 64 * 3 + 5
    dev = torch.device("cuda", 0)
    dR, dS = torch.from_numpy(R[:n].copy()).to(dev), torch.from_numpy(S[:n].copy()).to(dev)
    dK = torch.from_numpy(K[:n].astype(np.uint16).view(np.int16)).to(dev)
    mp = np.zeros(n * 85 + 64, np.uint8)
    mp[: n * 85] = M[:n].reshape(-1)
    dM = torch.from_numpy(mp).to(dev)
    dB = torch.zeros((n + 63) // 64, dtype=torch.int64, device=dev)
    gv.set_option(gv.OPT_COMB_BALANCE, 1)
    gv.reserve(n)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gv.verify_device(dR.data_ptr(), dS.data_ptr(), dK.data_ptr(), dM.data_ptr(), 85, 85, n, dB.data_ptr(),
                         torch.cuda.current_stream().cuda_stream)
    for rep in range(2):
        dB.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        bm = dB.cpu().numpy().view(np.uint64)
        assert (bitmap_to_bool(bm, n) == exp[:n]).all(), rep
        assert int(bm[-1]) >> (n % 64) == 0, rep


def test_balance_golden_corpus(chain4, batch, golden):
    """tests/golden's 85-byte batch (every adversarial class, keys the table build rejects), tiled past 2^16 rows
    so that the chain form takes it, once through the forced form: the committed expected bits."""
    gv = chain4
    pub = batch[0]
    b = dict(golden_batches(golden))[85]
    reps = -(-65536 // len(b["R"])) + 1
    R, S, M = (np.tile(b[k], (reps, 1)) for k in ("R", "S", "msg"))
    K = np.tile(b["key_idx"], reps)
    exp = np.tile(b["expected"].astype(bool), reps)
    n = len(R) - 37  # a partial last wave
    assert n > 65536 + 256
    try:
        ok = gv.set_keys(b["keys"])
        assert (ok == b["key_ok"].astype(bool)).all()
        for mode in (1, 0):
            gv.set_option(gv.OPT_COMB_BALANCE, mode)
            got, bm = verify(gv, R[:n], S[:n], K[:n], M[:n], 85)
            bad = np.nonzero(got != exp[:n])[0]
            assert len(bad) == 0, (mode, bad[:10], np.tile(b["cls"], reps)[bad[:10]])
            assert int(bm[-1]) >> (n % 64) == 0
    finally:
        assert gv.set_keys(pub).all()  # the module's key set, for whichever test runs next
