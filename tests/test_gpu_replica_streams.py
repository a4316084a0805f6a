"""pbft_replica_push_streams on the GPU: the differential test of tests/test_replica_streams.py on real signatures.
Replica A takes the host sequence (a forced flush, pbft_replica_push_frames per segment, a forced flush), replica B
the streams call, each on its own independently created context with the same keys (a context serves one replica);
the votes are signed on the GPU.  The streams stats say that B's calls ran the device chain -- index, decode, admit,
group, verify, two tallies -- and how many rows were clean and how many went to the per-frame host code."""
import ctypes

import numpy as np
import pytest

import streams_traffic as T
from test_gpu_verify import seeds_for
from test_replica_streams import Pair

pytestmark = pytest.mark.gpu
SEQS = [1, 2, 3, 4, 5, 6, 7, 8]


@pytest.fixture(scope="module")
def gvs():
    """Two independently created contexts (and a clone of the second), shared by the pairs of this module one after
    the other."""
    from pbft_amd import GpuBatchVerifier
    v = [GpuBatchVerifier(0), GpuBatchVerifier(0)]
    yield v
    for g in reversed(v):
        g.close()


class GpuPair(Pair):
    def __init__(self, gvs, n, multi=False):
        self.gvs = list(gvs[:2])
        self.seeds = seeds_for(n, tag=n)
        super().__init__(n, ctxs=[g._ctx for g in self.gvs], verifier=None)
        for g in self.gvs:
            assert g.set_keys(np.frombuffer(self.c.keys, np.uint8)).all()
        self.clone = None
        if multi:  # B again, over its context and a clone of it
            self.L.pbft_replica_destroy(self.B)
            self.clone = self.gvs[1].clone()
            ctxs = (ctypes.c_void_p * 2)(self.gvs[1]._ctx.value, self.clone._ctx.value)
            self.L.pbft_replica_create_multi.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                                         ctypes.c_uint32, ctypes.c_char_p,
                                                         ctypes.POINTER(ctypes.c_void_p)]
            r = ctypes.c_void_p()
            assert self.L.pbft_replica_create_multi(ctxs, 2, n, 0, self.c.keys, ctypes.byref(r)) == 0
            assert self.L.pbft_replica_set_log_window(r, T.WINDOW) == 0
            self.reps[1] = self.B = r

    def sign_batch(self, signers, env):
        R, S, pub = self.gvs[0].sign(self.seeds, signers, env, 85)
        assert pub.tobytes() == self.c.keys
        return np.concatenate([R, S], axis=1)

    def close(self):
        super().close()
        if self.clone is not None:
            self.clone.close()


@pytest.mark.parametrize("n", [4, 16])
def test_each_kind_and_all_together(gvs, n):
    """Every traffic kind alone on a fresh pair of replicas, then all of them merged: equal consumed, pushed, dropped,
    events, counters and predicates after every call, every call of B on the device path."""
    named = T.kinds(n, SEQS)
    for name, calls in list(named.items()) + [("together", T.together(named))]:
        p = GpuPair(gvs, n)
        try:
            p.run(calls, name)
            s = p.sstats()
            assert s["calls_device"] == len(calls) and s["calls_host_front"] == 0, (name, s)
            assert not any(v for k, v in s.items() if k.startswith("fallback_")), (name, s)
            if name == "honest":  # PrePrepares only in the residue; every vote clean, two envelopes per seq
                f = (n - 1) // 3
                live = n - f
                assert s["residue_rows"] == len(SEQS) and s["clean_rows"] == (2 * live - 1) * len(SEQS)
                assert s["envelopes"] == 2 * len(SEQS)
                assert all(p.L.pbft_replica_committed_local(p.B, T.VIEW, q) == 1 for q in SEQS)
            if name == "equivocation":  # the PrePrepare and the signer's three contested votes
                assert s["residue_rows"] == 4 and s["clean_rows"] == 1
            if name == "together":
                assert s["clean_rows"] > 0 and s["residue_rows"] > 20
        finally:
            p.close()


def test_fallbacks_on_the_device(gvs):
    """Caps below the traffic, after the device chain has run: the host sequence on the same bytes, equal results, the
    reason counted.  The same for a deferred vote that shares its key with a clean row.  And a replica of two contexts
    never takes the device path."""
    for reason, caps, hit in (("frames", (3, 64, 64), 2), ("envelopes", (4096, 1, 64), 2), ("residue", (4096, 64, 0), 1)):
        p = GpuPair(gvs, 4)
        try:
            assert p.L.pbft_replica_reserve_streams(p.B, 1 << 20, 64, *caps) == 0
            calls = T.kinds(4, SEQS)["honest"]
            p.run(calls, reason)
            s = p.sstats()
            assert s["fallback_" + reason] == hit and s["calls_device"] == len(calls) - hit, (reason, s)
        finally:
            p.close()
    p = GpuPair(gvs, 4)
    try:
        from test_replica_streams import twin_calls
        p.run(twin_calls(4), "twin")
        s = p.sstats()
        assert s["fallback_deferred"] == 1 and s["calls_device"] == 1, s
    finally:
        p.close()
    p = GpuPair(gvs, 4, multi=True)
    try:
        calls = T.kinds(4, SEQS)["honest"]
        p.run(calls, "multi")
        s = p.sstats()
        assert s["fallback_multi"] == len(calls) and s["calls_device"] == 0
    finally:
        p.close()


def test_reserved_sizes_serve_larger_streams(gvs):
    """pbft_replica_reserve_streams with room to spare, then two calls of different sizes on the device path."""
    p = GpuPair(gvs, 4)
    try:
        assert p.L.pbft_replica_reserve_streams(p.B, 1 << 20, 256, 2048, 256, 256) == 0
        p.run(T.together(T.kinds(4, SEQS)), "reserved")
        assert p.sstats()["calls_device"] == 3
    finally:
        p.close()
