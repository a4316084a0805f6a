"""Helpers of the proposal tests (test_propose.py, test_gpu_propose.py): the bindings of the replica's propose calls, a
deterministic mix of canonical and general client requests, the reference for a stream of signed PrePrepare frames --
hashlib's Blake2b-512 digests, the C oracle's RFC 8032 signatures over the kind-0 envelopes, pbft_wire_encode_preprepares
-- and a CPU proposer override built from them (pbft_replica_set_proposer)."""
import ctypes
import hashlib

import numpy as np

import egress_sim as E
from pbft_amd import wire

PROPOSE_LOOPBACK = 1
EINVAL = -1
# the decimal-width edges of tests/test_gpu_egress.py (VALS, REPLICAS)
VALS = [0, 9, 10, 99, 100, 2**32 - 1, 2**32, 10**19 - 1, 10**19, 2**64 - 1]
REPLICAS = [0, 9, 10, 999, 1000, 9999, 10000, 65534]
OP_LENS = [0, 1, 127, 128, 129, 3071, 3072, 3073]
SPECIALS = [b'"', b"\\", b"\x1f", b"\x7f", b"\xc3\xa9"]
C63 = "[2001:db8:85a3:8d3:1319:8a2e:370:7348%enp0s31f6-vlan1234567]:65535"[:63]
CLIENTS = ["127.0.0.1:8080", "10.0.0.7:1", "c", "127.0.0.1:8080", C63, "[::1]:9", "", "192.168.1.20:40000", C63 + "x",
           "127.0.0.1:8080"]
assert len(C63) == 63 and len(CLIENTS[8]) == 64
ALPHABET = np.array([c for c in range(0x20, 0x7F) if c not in (0x22, 0x5C)], np.uint8)

# (user, ops, ops_bytes, op_off, op_len, timestamp, clients, view, first_seq, n, replica, out, cap, len, digests, sigs)
PROPOSER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                               ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t,
                               ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p, ctypes.c_void_p)


class ProposeStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("proposed", "calls", "held_back", "loopback_applied", "propose_ns")]


def bind(L):
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    L.pbft_replica_propose.argtypes = [vp, u64, vp, u64, vp, vp, vp, vp, ctypes.c_uint32, vp, ctypes.c_size_t,
                                       ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(u64), ctypes.POINTER(u64)]
    L.pbft_replica_set_next_seq.argtypes = [vp, u64]
    L.pbft_replica_set_proposer.argtypes = [vp, PROPOSER_FN, vp]
    L.pbft_replica_get_propose_stats.argtypes = [vp, ctypes.POINTER(ProposeStats)]
    return L


def mixed_ops(n, salt=0):
    """n (operation, timestamp, client) triples: the operation lengths walk OP_LENS, a byte outside the canonical
    alphabet stands at the first or at the last byte of ten in every sixteen groups of eight, the clients walk CLIENTS
    (1, 63, 0 bytes and 64 bytes without a NUL among them), the timestamps walk VALS."""
    rng = np.random.default_rng(4000 + salt)
    ops, ts, cl = [], [], []
    for i in range(n):
        op = bytearray(ALPHABET[rng.integers(0, len(ALPHABET), OP_LENS[i % 8])].tobytes())
        s = (i // 8 + salt) % 16
        if s >= 6:
            sp = SPECIALS[(s - 6) // 2]
            if len(op) >= len(sp):
                if s % 2 == 0:
                    op[:len(sp)] = sp
                else:
                    op[len(op) - len(sp):] = sp
        ops.append(bytes(op))
        ts.append(VALS[(i + salt) % 10])
        cl.append(CLIENTS[(i * 7 // 5 + salt) % 10])
    return ops, ts, cl


def canonical(op, client):
    c = client.encode() if isinstance(client, str) else bytes(client)
    ok = lambda b: all(0x20 <= x <= 0x7E and x not in (0x22, 0x5C) for x in b)  # noqa: E731
    return len(op) <= 3072 and 1 <= len(c) <= 63 and ok(c) and ok(op)


def digests_of(ops):
    return np.stack([np.frombuffer(hashlib.blake2b(o, digest_size=64).digest(), np.uint8) for o in ops]) if ops else \
        np.zeros((0, 64), np.uint8)


def oracle_sigs(o, seed, view, first_seq, dig):
    """R || S [n][64] over pbft_envelope(0, view, first_seq + i, dig[i]) under `seed`, by the C oracle."""
    n = len(dig)
    env = E.envelopes([0] * n, [view] * n, [first_seq + i for i in range(n)], dig) if n else np.zeros((0, 85), np.uint8)
    return E.oracle_sign_batch(E.bind_oracle(o), seed, env) if n else np.zeros((0, 64), np.uint8)


def reference(o, seed, replica, view, first_seq, ops, ts, cl):
    """(requests, stream, frame_off, digests, sigs, status): what pbft_sign_preprepares_frames must return."""
    req = wire.pack_requests(ops, ts, cl)
    dig = digests_of(ops)
    sig = oracle_sigs(o, seed, view, first_seq, dig)
    stream, off, st = wire.encode_preprepares(view, first_seq, req, replica, dig, sig)
    return req, stream, off, dig, sig, st


def device_reference(stream, frame_off, status):
    """The device form's stream and frame_off: the reference restricted to the PROPOSE_OK requests."""
    lens = np.diff(frame_off.astype(np.int64))
    lens[status != 0] = 0
    parts = [stream[int(frame_off[i]):int(frame_off[i + 1])] for i in range(len(status)) if status[i] == 0]
    dev = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return dev, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def _arr(ptr, dtype, count):
    if count == 0:
        return np.zeros(0, dtype)
    raw = ctypes.string_at(ptr, count * np.dtype(dtype).itemsize)
    return np.frombuffer(raw, dtype).copy()


class OracleProposer:
    """pbft_replica_set_proposer override: hashlib digests, C-oracle signatures, pbft_wire_encode_preprepares."""

    def __init__(self, o, seed):
        self.o, self.seed, self.calls = o, seed, 0
        self.cb = PROPOSER_FN(self._propose)

    def install(self, L, rep):
        assert L.pbft_replica_set_proposer(rep, self.cb, None) == 0

    def _propose(self, user, ops, ops_bytes, op_off, op_len, ts, clients, view, first_seq, n, replica, out, cap, length,
                 digests, sigs):
        self.calls += 1
        n = int(n)
        off, ln = _arr(op_off, np.uint64, n), _arr(op_len, np.uint32, n)
        data = _arr(ops, np.uint8, int(ops_bytes))
        items = [data[int(a):int(a) + int(b)].tobytes() for a, b in zip(off, ln)]
        dig = digests_of(items)
        sg = oracle_sigs(self.o, self.seed, int(view), int(first_seq), dig)
        req = (np.concatenate([data, np.zeros(16, np.uint8)]), int(ops_bytes), off, ln, _arr(ts, np.uint64, n),
               _arr(clients, np.uint8, 64 * n).reshape(n, 64))
        stream, _, _ = wire.encode_preprepares(int(view), int(first_seq), req, int(replica), dig, sg)
        length[0] = len(stream)
        if len(stream) > cap:
            return EINVAL
        ctypes.memmove(out, stream.ctypes.data, len(stream))
        ctypes.memmove(digests, dig.ctypes.data, dig.size)
        ctypes.memmove(sigs, sg.ctypes.data, sg.size)
        return 0


def propose(L, rep, req, flags=0, cap=None, count=None):
    """(rc, stream or None, len, first_seq, n_proposed): the size query first unless a cap is given."""
    data, ops_bytes, off, ln, ts, cl = req
    n = len(ln) if count is None else count
    need, first, np_ = ctypes.c_size_t(), ctypes.c_uint64(), ctypes.c_uint64()
    args = (rep, n, data.ctypes.data, ops_bytes, off.ctypes.data, ln.ctypes.data, ts.ctypes.data, cl.ctypes.data)
    if cap is None:
        assert L.pbft_replica_propose(*args, 0, None, 0, ctypes.byref(need), ctypes.byref(first), ctypes.byref(np_)) == 0
        cap = need.value
    buf = np.zeros(max(cap, 1), np.uint8)
    rc = L.pbft_replica_propose(*args, flags, buf.ctypes.data if cap else None, cap, ctypes.byref(need),
                                ctypes.byref(first), ctypes.byref(np_))
    return rc, (buf[:need.value].copy() if rc == 0 else None), need.value, first.value, np_.value


def propose_stats(L, rep):
    s = ProposeStats()
    assert L.pbft_replica_get_propose_stats(rep, ctypes.byref(s)) == 0
    return {k: getattr(s, k) for k, _ in ProposeStats._fields_}


def slice_requests(req, lo, hi):
    """Requests [lo, hi) of a pack_requests tuple, over the same operation bytes."""
    data, ops_bytes, off, ln, ts, cl = req
    return data, ops_bytes, off[lo:hi].copy(), ln[lo:hi].copy(), ts[lo:hi].copy(), cl[lo:hi].copy()
