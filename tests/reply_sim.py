"""Helpers of the reply tests (test_reply.py, test_gpu_reply.py): the bindings of the replica's reply calls, a
deterministic mix of canonical and general results, the reference for a stream of signed client replies -- hashlib's
Blake2b-512 over C | result, the C oracle's RFC 8032 signatures over the kind-3 envelopes, pbft_wire_encode_replies -- and
a CPU replier override built from them (pbft_replica_set_replier)."""
import ctypes
import hashlib

import numpy as np

import egress_sim as E
from pbft_amd import wire

EINVAL = -1
VALS = [0, 9, 10, 99, 100, 2**32 - 1, 2**32, 10**19 - 1, 10**19, 2**64 - 1]
RES_LENS = [0, 1, 63, 64, 65, 191, 192, 193, 3071, 3072, 3073]  # 64 + len = 128 and 256: the hash's block boundaries
SPECIALS = [b'"', b"\\", b"\x1f", b"\x7f", b"\xc3\xa9"]
C63 = "[2001:db8:85a3:8d3:1319:8a2e:370:7348%enp0s31f6-vlan1234567]:65535"[:63]
# a client with bytes behind its NUL, and one without a NUL
CLIENTS = [b"127.0.0.1:8080", b"10.0.0.7:1", b"c", C63.encode(), b"[::1]:9\0junk behind the NUL", b"", (C63 + "x").encode(),
           b"192.168.1.20:40000"]
ALPHABET = np.array([c for c in range(0x20, 0x7F) if c not in (0x22, 0x5C)], np.uint8)

# (user, results, results_bytes, res_off, res_len, timestamp, clients, view, n, replica, out, cap, len)
REPLIER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                              ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t))


class ReplyStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("replied", "calls", "stale", "not_committed", "reply_ns")]


def bind(L):
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    L.pbft_replica_reply.argtypes = [vp, u64, vp, vp, vp, vp, u64, vp, vp, ctypes.c_uint32, vp, ctypes.c_size_t,
                                     ctypes.POINTER(ctypes.c_size_t), vp, vp, ctypes.POINTER(u64)]
    L.pbft_replica_set_replier.argtypes = [vp, REPLIER_FN, vp]
    L.pbft_replica_set_last_timestamp.argtypes = [vp, u64]
    L.pbft_replica_last_timestamp.argtypes = [vp, ctypes.POINTER(u64)]
    L.pbft_replica_get_reply_stats.argtypes = [vp, ctypes.POINTER(ReplyStats)]
    L.pbft_reply_envelope.argtypes = [ctypes.c_char_p, u64, u64, ctypes.c_char_p]
    L.pbft_reply_envelope.restype = None
    L.pbft_peer_id_b58_from_key.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    L.pbft_key_from_peer_id_b58.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    return L


def public_key(o, seed):
    b = ctypes.create_string_buffer(32)
    o.oracle_public_key.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    o.oracle_public_key(b, bytes(seed))
    return b.raw


def mixed_results(n, salt=0, general=True):
    """n (result, timestamp, client) triples: the result lengths walk RES_LENS (without 3073 unless `general`), a byte
    outside the canonical alphabet stands at the first, a middle or the last position in five of every eight groups of
    eleven (only if `general`), the clients walk CLIENTS, the timestamps walk VALS."""
    rng = np.random.default_rng(7000 + salt)
    lens = RES_LENS if general else RES_LENS[:-1]
    res, ts, cl = [], [], []
    for i in range(n):
        r = bytearray(ALPHABET[rng.integers(0, len(ALPHABET), lens[i % len(lens)])].tobytes())
        s = (i // len(lens) + salt) % 8
        if general and s >= 3:
            sp = SPECIALS[s - 3]
            if len(r) >= len(sp):
                at = [0, (len(r) - len(sp)) // 2, len(r) - len(sp)][i % 3]
                r[at:at + len(sp)] = sp
        res.append(bytes(r))
        ts.append(VALS[(i + salt) % 10])
        cl.append(CLIENTS[(i * 3 + salt) % len(CLIENTS)])
    return res, ts, cl


def digests_of(results, clients):
    """hashlib's D = Blake2b-512(C | result), uint8[n][64]."""
    if not results:
        return np.zeros((0, 64), np.uint8)
    return np.stack([np.frombuffer(hashlib.blake2b(wire.client_field(c) + bytes(r), digest_size=64).digest(), np.uint8)
                     for r, c in zip(results, clients)])


def envelopes(L, view, ts, dig):
    """[n][85] by pbft_reply_envelope."""
    out = np.zeros((len(ts), 85), np.uint8)
    for i, t in enumerate(ts):
        b = ctypes.create_string_buffer(85)
        L.pbft_reply_envelope(b, view, int(t), dig[i].tobytes())
        out[i] = np.frombuffer(b.raw, np.uint8)
    return out


def oracle_sigs(L, o, seed, view, ts, dig):
    """R || S [n][64] over pbft_reply_envelope(view, ts[i], dig[i]) under `seed`, by the C oracle's RFC 8032 signer."""
    n = len(ts)
    return E.oracle_sign_batch(E.bind_oracle(o), seed, envelopes(L, view, ts, dig)) if n else np.zeros((0, 64), np.uint8)


def reference(L, o, seed, replica, view, results, ts, cl):
    """(requests, stream, reply_off, digests, sigs, status): what pbft_sign_replies must return."""
    req = wire.pack_results(results, ts, cl)
    dig = digests_of(results, cl)
    sig = oracle_sigs(L, o, seed, view, ts, dig)
    stream, off, st = wire.encode_replies(view, req, replica, wire.peer_id_b58(public_key(o, seed)), sig)
    return req, stream, off, dig, sig, st


def device_reference(stream, reply_off, status):
    """The device form's stream and reply_off: the reference restricted to the REPLY_OK replies."""
    lens = np.diff(reply_off.astype(np.int64))
    lens[status != 0] = 0
    parts = [stream[int(reply_off[i]):int(reply_off[i + 1])] for i in range(len(status)) if status[i] == 0]
    dev = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return dev, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def _arr(ptr, dtype, count):
    if count == 0:
        return np.zeros(0, dtype)
    raw = ctypes.string_at(ptr, count * np.dtype(dtype).itemsize)
    return np.frombuffer(raw, dtype).copy()


class OracleReplier:
    """pbft_replica_set_replier override: hashlib digests, C-oracle signatures, pbft_wire_encode_replies."""

    def __init__(self, L, o, seed):
        self.L, self.o, self.seed, self.calls = L, o, seed, 0
        self.pid = wire.peer_id_b58(public_key(o, seed))
        self.cb = REPLIER_FN(self._reply)

    def install(self, L, rep):
        assert L.pbft_replica_set_replier(rep, self.cb, None) == 0

    def _reply(self, user, results, results_bytes, res_off, res_len, ts, clients, view, n, replica, out, cap, length):
        self.calls += 1
        n = int(n)
        off, ln, t = _arr(res_off, np.uint64, n), _arr(res_len, np.uint32, n), _arr(ts, np.uint64, n)
        data = _arr(results, np.uint8, int(results_bytes))
        cl = _arr(clients, np.uint8, 64 * n).reshape(n, 64)
        items = [data[int(a):int(a) + int(b)].tobytes() for a, b in zip(off, ln)]
        dig = digests_of(items, [c.tobytes() for c in cl])
        sg = oracle_sigs(self.L, self.o, self.seed, int(view), t, dig)
        req = (np.concatenate([data, np.zeros(16, np.uint8)]), int(results_bytes), off, ln, t, cl)
        stream, _, _ = wire.encode_replies(int(view), req, int(replica), self.pid, sg)
        length[0] = len(stream)
        if len(stream) > cap:
            return EINVAL
        ctypes.memmove(out, stream.ctypes.data, len(stream))
        return 0


def reply(L, rep, seqs, req, cap=None, flags=0):
    """(rc, stream or None, len, reply_off, status, n_replied): the size query first unless a cap is given."""
    data, nbytes, off, ln, ts, cl = req
    n = len(ln)
    sq = np.ascontiguousarray(seqs, np.uint64)
    need, nr = ctypes.c_size_t(), ctypes.c_uint64()
    roff, st = np.zeros(n + 1, np.uint64), np.full(max(n, 1), 0xEE, np.uint8)
    args = (rep, n, sq.ctypes.data, ts.ctypes.data, cl.ctypes.data, data.ctypes.data, nbytes, off.ctypes.data,
            ln.ctypes.data)
    if cap is None:
        assert L.pbft_replica_reply(*args, 0, None, 0, ctypes.byref(need), None, None, ctypes.byref(nr)) == 0
        cap = need.value
    buf = np.zeros(max(cap, 1), np.uint8)
    rc = L.pbft_replica_reply(*args, flags, buf.ctypes.data if cap else None, cap, ctypes.byref(need), roff.ctypes.data,
                              st.ctypes.data, ctypes.byref(nr))
    return rc, (buf[:need.value].copy() if rc == 0 else None), need.value, roff, st[:n], nr.value


def reply_stats(L, rep):
    s = ReplyStats()
    assert L.pbft_replica_get_reply_stats(rep, ctypes.byref(s)) == 0
    return {k: getattr(s, k) for k, _ in ReplyStats._fields_}


def last_timestamp(L, rep):
    v = ctypes.c_uint64()
    assert L.pbft_replica_last_timestamp(rep, ctypes.byref(v)) == 0
    return v.value
