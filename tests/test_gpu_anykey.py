"""Verification under uninstalled keys on the GPU (run with -m gpu on an MI355X): pbft_verify_batch_keys and its device
form on a context WITHOUT a key set against the golden corpus, the C oracle and the table path; ragged batch sizes with
every signature under its own key; the point hook against oracle/ed25519_ref.py; the base-point part's edge digits; a
hipGraph capture."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import anykey_cases as C
import comb_edges as CE
from conftest import ROOT

pytestmark = pytest.mark.gpu
L = C.L
N_MAX = 4096 + 77
SIZES = (1, 63, 64, 65, N_MAX)


@pytest.fixture(scope="module")
def gv():
    """A context that never gets a key set."""
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
    lib.oracle_sign_batch.argtypes = [vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, vp, vp,
                                      ctypes.c_int]
    lib.oracle_public_key.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    return lib


def bits_of(bm, n):
    from pbft_amd import bitmap_to_bool
    return bitmap_to_bool(np.asarray(bm).view(np.uint64), n)


def device_run(gv, R, S, A, msg, msg_len, extra_words=2, graph=False):
    """The device form with the bitmap (and extra_words past it) prefilled with ones: (bits, the raw words)."""
    import torch
    dev = torch.device("cuda", 0)
    n, stride = len(R), msg.shape[1]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    mp = np.zeros(n * stride + 64, np.uint8)
    mp[: n * stride] = np.ascontiguousarray(msg).reshape(-1)
    dR, dS, dA, dM = up(R), up(S), up(A), up(mp)
    words = (n + 63) // 64
    dB = torch.full((words + extra_words,), -1, dtype=torch.int64, device=dev)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        gv.verify_keys_device(dR.data_ptr(), dS.data_ptr(), dA.data_ptr(), dM.data_ptr(), msg_len, stride, n,
                              dB.data_ptr(), st.cuda_stream)
    torch.cuda.synchronize()
    w = dB.cpu().numpy().view(np.uint64)
    return bits_of(w[:words], n), w


def check_words(w, n, where):
    words = (n + 63) // 64
    assert (w[words:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), ("words past the batch were written", where)
    if n % 64:
        assert int(w[words - 1]) >> (n % 64) == 0, ("bits past N", where)


# ---- the golden corpus, no key set installed ----
def test_golden_corpus_without_a_key_set(gv):
    from pbft_amd import PbftError, SigBatch
    with pytest.raises(PbftError) as e:  # (the table path has nothing to verify against on this context)
        gv.verify(SigBatch(np.zeros((1, 32), np.uint8), np.zeros((1, 32), np.uint8), np.zeros(1, np.uint16),
                           np.zeros((1, 85), np.uint8), 85))
    assert e.value.code == -3
    lens = set()
    for ml, R, S, A, msg, exp in C.golden_inline():
        n = len(R)
        host = gv.verify_keys(R, S, A, msg, ml)
        got = bits_of(host, n)
        assert (got == exp).all(), (ml, "host", np.nonzero(got != exp)[0][:10])
        if n % 64:
            assert int(host[-1]) >> (n % 64) == 0
        got, w = device_run(gv, R, S, A, msg, ml)
        assert (got == exp).all(), (ml, "device", np.nonzero(got != exp)[0][:10])
        check_words(w, n, ml)
        lens.add(ml)
    assert 85 in lens and len(lens) == 11  # both instances of the kernel: 85 bytes and any length


def test_golden_corpus_equals_the_table_path():
    """Each batch's keys installed on a second context: the table path's bits are the inline path's, and installing
    keys does not change what the inline path returns."""
    from pbft_amd import GpuBatchVerifier, SigBatch
    g = np.load(os.path.join(C.GOLDEN, "verify_vectors.npz"))
    v = GpuBatchVerifier(0)
    try:
        for (ml, b), (_, R, S, A, msg, exp) in zip(C.golden_batches(g), C.golden_inline()):
            n = len(R)
            v.set_keys(b["keys"])
            table = bits_of(v.verify(SigBatch(b["R"], b["S"], b["key_idx"], b["msg"], ml)), n)
            inline = bits_of(v.verify_keys(R, S, A, msg, ml), n)
            assert (table == inline).all() and (inline == exp).all(), ml
            again = bits_of(v.verify(SigBatch(b["R"], b["S"], b["key_idx"], b["msg"], ml)), n)
            assert (again == table).all(), ml  # (the installed set was not disturbed)
    finally:
        v.close()


# ---- ragged sizes, every signature under its own key ----
def key_seed(i):
    return hashlib.sha512(b"pbft-key" + (77).to_bytes(8, "little") + i.to_bytes(8, "little")).digest()[:32]


@pytest.fixture(scope="module")
def own_keys(coracle):
    """N_MAX signatures, signature i under key i; 1 % of the lanes (and a few inside the first 65) mutated over the
    golden classes that need no special key; the C oracle's bits.  The smaller sizes are prefixes."""
    n = N_MAX
    seeds = np.frombuffer(b"".join(key_seed(i) for i in range(n)), np.uint8).reshape(n, 32).copy()
    pub = np.zeros((n, 32), np.uint8)
    for i in range(n):
        out = ctypes.create_string_buffer(32)
        coracle.oracle_public_key(out, seeds[i].tobytes())
        pub[i] = np.frombuffer(out.raw, np.uint8)
    msg = np.zeros((n, 85), np.uint8)
    for i in range(n):
        d = hashlib.blake2b(b"req-" + str(i // 7).encode(), digest_size=64).digest()
        msg[i] = np.frombuffer(b"PBFT" + bytes([1 + i % 2]) + (3).to_bytes(8, "little") + (i // 7).to_bytes(8, "little") + d,
                               np.uint8)
    idx = np.arange(n, dtype=np.uint16)
    R, S = np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8)
    assert coracle.oracle_sign_batch(seeds.ctypes.data, idx.ctypes.data, msg.ctypes.data, 85, 85, n, R.ctypes.data,
                                     S.ctypes.data, min(16, os.cpu_count() or 1)) == 0
    A = pub.copy()
    rng = np.random.default_rng(16)
    lanes = np.unique(np.concatenate([[0, 3, 17, 40, 62, 63, 64], rng.choice(n, size=n // 100, replace=False)]))
    so = [bytes.fromhex(h) for h in C.KAT["small_order_encodings"]]
    nc = [bytes.fromhex(h) for h in C.KAT["noncanonical_decodable_encodings"]]
    row = lambda b: np.frombuffer(b, np.uint8)  # noqa: E731
    for j, i in enumerate(lanes):
        c = j % 11
        if c == 0:
            msg[i, rng.integers(85)] ^= 1 << rng.integers(8)
        elif c == 1:
            R[i, rng.integers(32)] ^= 1 << rng.integers(8)
        elif c == 2:
            S[i, rng.integers(32)] ^= 1 << rng.integers(8)
        elif c == 3:
            S[i] = row((int.from_bytes(S[i].tobytes(), "little") + L).to_bytes(32, "little"))
        elif c == 4:
            S[i, 31] |= 0x80
        elif c == 5:
            R[i] = row((2).to_bytes(32, "little"))  # not on the curve
        elif c == 6:
            R[i] = row(nc[j % len(nc)])
        elif c == 7:
            R[i] = row(so[j % len(so)])
        elif c == 8:
            A[i] = pub[(i + 1) % n]  # another signer's key
        elif c == 9:
            R[i] = 0
            S[i] = 0
        else:  # s >= 2^253: rejected, and recoded as 0
            S[i, 31] |= (0x20, 0x40, 0xE0)[j % 3]
    exp = np.zeros(n, np.uint8)
    assert coracle.oracle_verify_batch(A.ctypes.data, n, R.ctypes.data, S.ctypes.data, idx.ctypes.data, msg.ctypes.data,
                                       85, 85, n, exp.ctypes.data, min(16, os.cpu_count() or 1)) == 0
    exp = exp.astype(bool)
    keep = np.ones(n, bool)
    keep[lanes] = False
    assert not exp[lanes].any() and exp[keep].all() and len(np.unique(pub, axis=0)) == n
    return R, S, A, msg, exp


@pytest.mark.parametrize("n", SIZES)
def test_ragged_sizes_each_signature_under_its_own_key(gv, own_keys, n):
    R, S, A, msg, exp = (x[:n] for x in own_keys)
    host = gv.verify_keys(R, S, A, msg, 85)
    assert len(host) == (n + 63) // 64
    got = bits_of(host, n)
    assert (got == exp).all(), ("host", np.nonzero(got != exp)[0][:10])
    if n % 64:
        assert int(host[-1]) >> (n % 64) == 0
    got, w = device_run(gv, R, S, A, msg, 85)
    assert (got == exp).all(), ("device", np.nonzero(got != exp)[0][:10])
    check_words(w, n, n)


# ---- the point hook ----
def test_point_hook_on_the_gpu(gv):
    s, k, A, enc, kok, dec = C.point_cases()
    if len(s) % 64 == 0:  # a partial last wave
        s, k, A, enc, kok, dec = (np.concatenate([x, x[:13]]) for x in (s, k, A, enc, kok, dec))
    assert len(s) % 64 and len(s) > 77
    got, got_ok = gv.debug_anykey_point(s, k, A)
    assert (got_ok == kok).all(), np.nonzero(got_ok != kok)[0][:10]
    d = dec.astype(bool)
    bad = np.nonzero((got[d] != enc[d]).any(axis=1))[0]
    assert len(bad) == 0, bad[:10]
    # one item alone: the dead lanes of its wave recompute it
    one, one_ok = gv.debug_anykey_point(s[5:6], k[5:6], A[5:6])
    assert (one[0] == enc[5]).all() and one_ok[0] == kok[5]


# ---- the base-point part at its edge digits ----
def test_edge_digits_of_s_under_the_base_plan(gv):
    fx = CE.load()
    rows = np.nonzero(fx["plan"] == 0)[0]
    assert len(rows) > 50 and fx["twin"][rows].any() and not fx["twin"][rows].all()
    R, S, msg = fx["R"][rows], fx["S"][rows], fx["msg"][rows]
    A = np.tile(fx["key"], (len(rows), 1))
    exp = fx["expected"][rows].astype(bool)
    got = bits_of(gv.verify_keys(R, S, A, msg, 85), len(rows))
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, CE.describe(fx, rows[bad[:10]])
    assert (exp == ~fx["twin"][rows].astype(bool)).all()


# ---- hipGraph ----
def test_device_form_captured_in_a_hip_graph(gv):
    """After pbft_verify_reserve the device form is captured on one stream -- two kernel nodes, one after the other,
    no memset node -- and replayed twice over a bitmap refilled with ones."""
    import torch
    ml, R, S, A, msg, exp = next(b for b in C.golden_inline() if b[0] == 85)
    n = len(R)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    mp = np.zeros(n * 85 + 64, np.uint8)
    mp[: n * 85] = msg.reshape(-1)
    dR, dS, dA, dM = up(R), up(S), up(A), up(mp)
    words = (n + 63) // 64
    dB = torch.full((words + 2,), -1, dtype=torch.int64, device=dev)
    gv.reserve(n)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gv.verify_keys_device(dR.data_ptr(), dS.data_ptr(), dA.data_ptr(), dM.data_ptr(), 85, 85, n, dB.data_ptr(),
                              torch.cuda.current_stream().cuda_stream)
    for rep in range(2):
        dB.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        w = dB.cpu().numpy().view(np.uint64)
        assert (bits_of(w[:words], n) == exp).all(), rep
        check_words(w, n, rep)


def test_arguments(gv):
    z =np.zeros((4, 32), np.uint8)
    assert len(gv.verify_keys(z[:0], z[:0], z[:0], np.zeros((0, 85), np.uint8), 85)) == 0
    out = np.zeros(3, np.uint64)
    lib, p = gv._lib, z.ctypes.data
    assert lib.pbft_verify_batch_keys(gv._ctx, p, p, p, p, 85, 32, 4, out.ctypes.data) == -1  # msg_stride < msg_len
    assert lib.pbft_verify_batch_keys(gv._ctx, p, p, None, p, 32, 32, 4, out.ctypes.data) == -1  # no keys
    assert lib.pbft_verify_batch_keys_device(gv._ctx, p, p, p, p, 85, 32, 4, out.ctypes.data, None) == -1
    assert lib.pbft_verify_batch_keys_device(gv._ctx, p, p, p, p, 32, 32, 4, None, None) == -1
    with pytest.raises(ValueError):
        gv.verify_keys(z, z, z[:3], np.zeros((4, 85), np.uint8), 85)
    assert not out.any()
