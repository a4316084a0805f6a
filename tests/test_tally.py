"""The vote tally's boundary that needs no GPU: the library exports pbft_tally_device and pbft_verify_votes_tally, a
null context is an error (not a crash), and tally_reference -- the numpy statement of the semantics the GPU tests
compare against -- equals a brute-force loop over the rows."""
import numpy as np
import pytest


def brute_force(bits, key_idx, env_idx, n_env, n_signers):
    W = (n_signers + 63) // 64
    sets = [set() for _ in range(n_env)]
    for b, k, e in zip(bits, key_idx, env_idx):
        if b and e < n_env and k < n_signers:
            sets[int(e)].add(int(k))
    signers = np.zeros((n_env, W), dtype=np.uint64)
    for e, s in enumerate(sets):
        for k in s:
            signers[e, k // 64] |= np.uint64(1 << (k % 64))
    return signers, np.array([len(s) for s in sets], dtype=np.uint32)


def random_case(rng, n, n_env, n_signers):
    """Rows with duplicated (signer, envelope) pairs and ~5 % of each index out of range with the bit set."""
    key_idx = rng.integers(0, n_signers, n).astype(np.uint16)
    env_idx = rng.integers(0, n_env, n).astype(np.uint32)
    bits = rng.random(n) < 0.7
    if n >= 4:  # exact duplicates of earlier rows, bit set on both
        dup = rng.integers(0, n // 2, n // 4)
        key_idx[n // 2: n // 2 + len(dup)] = key_idx[dup]
        env_idx[n // 2: n // 2 + len(dup)] = env_idx[dup]
        bits[dup] = True
        bits[n // 2: n // 2 + len(dup)] = True
    bad_e = rng.random(n) < 0.05
    env_idx[bad_e] = n_env + rng.integers(0, 3, int(bad_e.sum())).astype(np.uint32)
    bad_k = rng.random(n) < 0.05
    key_idx[bad_k] = np.minimum(n_signers + rng.integers(0, 70, int(bad_k.sum())), 65535).astype(np.uint16)
    bits[bad_e | bad_k] = True
    return bits, key_idx, env_idx


def test_library_exports_the_tally():
    import pbft_amd
    lib = pbft_amd.load()
    for f in ("pbft_tally_device", "pbft_verify_votes_tally"):
        assert hasattr(lib, f), f
        assert f in pbft_amd.EXPORTS


def test_null_context_is_an_error():
    import pbft_amd
    lib = pbft_amd.load()
    assert lib.pbft_tally_device(None, None, None, 2, None, 4, 0, 0, 4, 0, None, None, None) == -1
    assert lib.pbft_verify_votes_tally(None, None, None, None, None, None, 0, 0, None, None, None) == -1


@pytest.mark.parametrize("n_signers", [1, 64, 65, 1000])
@pytest.mark.parametrize("n,n_env", [(0, 3), (1, 1), (200, 7), (3000, 40)])
def test_reference_equals_brute_force(n_signers, n, n_env):
    from pbft_amd import quorum, tally_reference
    rng = np.random.default_rng(1000 * n_signers + n)
    bits, key_idx, env_idx = random_case(rng, n, n_env, n_signers)
    signers, counts = tally_reference(bits, key_idx, env_idx, n_env, n_signers)
    exp_s, exp_c = brute_force(bits, key_idx, env_idx, n_env, n_signers)
    assert signers.dtype == np.uint64 and signers.shape == (n_env, (n_signers + 63) // 64)
    assert counts.dtype == np.uint32 and counts.shape == (n_env,)
    assert (signers == exp_s).all() and (counts == exp_c).all()
    # bits at or above n_signers of the last word stay 0
    if n_signers % 64:
        assert not (signers[:, -1] >> np.uint64(n_signers % 64)).any()
    assert (quorum(counts, 2) == (exp_c >= 2)).all()


def test_reference_duplicates_and_out_of_range():
    from pbft_amd import tally_reference
    #        valid   dup     bit 0   env out  key out  other env
    bits = [True, True, False, True, True, True]
    key = [3, 3, 5, 1, 70, 65]
    env = [0, 0, 0, 2, 1, 1]
    signers, counts = tally_reference(bits, key, env, 2, 66)
    assert counts.tolist() == [1, 1]
    assert signers.tolist() == [[1 << 3, 0], [0, 1 << 1]]
