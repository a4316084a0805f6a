"""Helpers of the egress tests (test_egress.py, test_gpu_egress.py): the bindings of the replica's egress calls, the
reference for a stream of signed vote frames -- the C oracle's RFC 8032 signatures encoded by pbft_wire_encode_votes --
and a CPU signer override built from the two (pbft_replica_set_signer)."""
import ctypes

import numpy as np

EMIT_LOOPBACK = 1
EINVAL = -1
# (user, envelopes[N][85], N, replica, out, cap, len, sigs[N][64])
SIGNER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
                             ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p)


class EgressStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("queued", "emitted", "calls", "loopback_pushed", "emit_ns")]


def bind(L):
    vp = ctypes.c_void_p
    L.pbft_replica_set_signing_seed.argtypes = [vp, ctypes.c_char_p]
    L.pbft_replica_set_signer.argtypes = [vp, SIGNER_FN, vp]
    L.pbft_replica_emit_frames.argtypes = [vp, ctypes.c_uint32, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                                           ctypes.POINTER(ctypes.c_uint64)]
    L.pbft_replica_get_egress_stats.argtypes = [vp, ctypes.POINTER(EgressStats)]
    return L


def bind_oracle(o):
    vp = ctypes.c_void_p
    o.oracle_sign_batch.argtypes = [vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, vp, vp, ctypes.c_int]
    return o


def envelopes(kind, view, seq, digests):
    """[N][85]: "PBFT" | kind | view LE | seq LE | digest (pbft_envelope)."""
    n = len(kind)
    e = np.zeros((n, 85), np.uint8)
    e[:, :4] = np.frombuffer(b"PBFT", np.uint8)
    e[:, 4] = np.asarray(kind, np.uint8)
    e[:, 5:13] = np.asarray(view, "<u8").reshape(n, 1).view(np.uint8)
    e[:, 13:21] = np.asarray(seq, "<u8").reshape(n, 1).view(np.uint8)
    e[:, 21:] = np.asarray(digests, np.uint8).reshape(n, 64)
    return e


def fields(env):
    env = np.ascontiguousarray(env, np.uint8).reshape(-1, 85)
    return (env[:, 4].copy(), env[:, 5:13].copy().view("<u8").reshape(-1), env[:, 13:21].copy().view("<u8").reshape(-1),
            env[:, 21:].copy())


def valid_mask(env):
    env = np.ascontiguousarray(env, np.uint8).reshape(-1, 85)
    return (env[:, :4] == np.frombuffer(b"PBFT", np.uint8)).all(axis=1) & ((env[:, 4] == 1) | (env[:, 4] == 2))


def oracle_sign_batch(o, seed, env):
    """R || S [N][64] of the N envelopes under `seed`, by the C oracle."""
    env = np.ascontiguousarray(env, np.uint8).reshape(-1, 85)
    n = len(env)
    sd = np.frombuffer(bytes(seed), np.uint8).copy()
    idx = np.zeros(max(n, 1), np.uint16)
    R, S = np.zeros((max(n, 1), 32), np.uint8), np.zeros((max(n, 1), 32), np.uint8)
    if n:
        assert o.oracle_sign_batch(sd.ctypes.data, idx.ctypes.data, env.ctypes.data, 85, 85, n, R.ctypes.data,
                                   S.ctypes.data, 4) == 0
    return np.concatenate([R[:n], S[:n]], axis=1)


def oracle_frames(o, seed, replica, env):
    """(stream, frame_off [N + 1], sigs [N][64]) the library must produce for the envelopes: the frames of the valid
    ones, oracle-signed and encoded by pbft_wire_encode_votes; an invalid envelope has length 0 and a zero signature."""
    from pbft_amd import wire
    env = np.ascontiguousarray(env, np.uint8).reshape(-1, 85)
    ok = valid_mask(env)
    sigs = np.zeros((len(env), 64), np.uint8)
    sigs[ok] = oracle_sign_batch(o, seed, env[ok])
    kind, view, seq, dig = fields(env[ok])
    m = int(ok.sum())
    stream = wire.encode_votes(kind, view, seq, dig, np.full(m, replica, np.uint32), sigs[ok]) if m else \
        np.zeros(0, np.uint8)
    off, flen, used = wire.frame_index(stream) if m else (np.zeros(0, np.uint64), np.zeros(0, np.uint32), 0)
    assert used == len(stream) and len(off) == m
    lens = np.zeros(len(env), np.uint64)
    lens[ok] = flen.astype(np.uint64) + 2  # (every vote's varint has two bytes)
    frame_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    assert int(frame_off[-1]) == len(stream)
    return stream, frame_off, sigs


class OracleSigner:
    """pbft_replica_set_signer override: signs with the C oracle, encodes with pbft_wire_encode_votes."""

    def __init__(self, o, seed):
        self.o, self.seed, self.calls = bind_oracle(o), seed, 0
        self.cb = SIGNER_FN(self._sign)

    def install(self, L, rep):
        assert L.pbft_replica_set_signer(rep, self.cb, None) == 0

    def _sign(self, user, envs, n, replica, out, cap, length, sigs):
        self.calls += 1
        n = int(n)
        env = np.ctypeslib.as_array(ctypes.cast(envs, ctypes.POINTER(ctypes.c_uint8)), (n * 85,)).reshape(n, 85).copy()
        stream, _, sg = oracle_frames(self.o, self.seed, int(replica), env)
        length[0] = len(stream)
        if len(stream) > cap:
            return EINVAL
        ctypes.memmove(out, stream.ctypes.data, len(stream))
        ctypes.memmove(sigs, sg.ctypes.data, sg.size)
        return 0


def emit(L, rep, flags=0, cap=None):
    """(rc, stream bytes or None, len, n_votes): the size query first unless a cap is given."""
    need, nv = ctypes.c_size_t(), ctypes.c_uint64()
    if cap is None:
        assert L.pbft_replica_emit_frames(rep, 0, None, 0, ctypes.byref(need), ctypes.byref(nv)) == 0
        assert nv.value == 0
        cap = need.value
    buf = np.zeros(max(cap, 1), np.uint8)
    rc = L.pbft_replica_emit_frames(rep, flags, buf.ctypes.data if cap else None, cap, ctypes.byref(need),
                                    ctypes.byref(nv))
    return rc, (buf[:need.value].copy() if rc == 0 else None), need.value, nv.value


def egress_stats(L, rep):
    s = EgressStats()
    assert L.pbft_replica_get_egress_stats(rep, ctypes.byref(s)) == 0
    return {k: getattr(s, k) for k, _ in EgressStats._fields_}
