"""Helpers of the acceptance tests (test_accept.py, test_gpu_accept.py): a corpus of signed client replies from n = 4
replicas to 3 clients -- an honest base (every replica answers every request; pbft_wire_encode_replies' texts with the C
oracle's RFC 8032 signatures, tests/reply_sim.py) with the cases planted that a client has to survive -- and the
model's answer for it (pbft_amd.accept_reference with the oracle's verify_strict)."""
import ctypes
import hashlib
import os

import numpy as np

import reply_sim as R
from conftest import ROOT
from pbft_amd import accept_reference, wire

N_REPLICAS, F, NEED = 4, 1, 2
SEEDS = [hashlib.sha512(b"accept-replica-%d" % i).digest()[:32] for i in range(N_REPLICAS)]
CLIENTS = [b"127.0.0.1:8080", b"10.0.0.7:1", R.C63.encode()]
RES_LENS = [0, 1, 63, 64, 65, 191, 192, 193, 3071, 3072]
GENERAL = [b'a "quoted" result', b"back\\slash", b"two\nlines", "café résulté".encode()]

_world = None


class World:
    def __init__(self):
        o = ctypes.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))
        o.oracle_public_key.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
        o.oracle_sign.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
        o.oracle_sign.restype = None
        o.oracle_verify_strict.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
        self.o, self.L = o, R.bind(wire.load())
        self.pubs = [R.public_key(o, s) for s in SEEDS]
        self.pids = [wire.peer_id_b58(p) for p in self.pubs]
        self.keys = np.frombuffer(b"".join(self.pubs), np.uint8).reshape(N_REPLICAS, 32).copy()

    def sign(self, seed, env):
        b = ctypes.create_string_buffer(64)
        self.o.oracle_sign(b, bytes(seed), bytes(env), len(env))
        return b.raw

    def verify_with(self, pubs):
        return lambda rep, sig, env: self.o.oracle_verify_strict(bytes(pubs[rep]), sig, env, len(env)) == 1

    @property
    def verify(self):
        return self.verify_with(self.pubs)


def world():
    global _world
    if _world is None:
        _world = World()
    return _world


def envelope(view, ts, client, result):
    d = hashlib.blake2b(wire.client_field(client) + bytes(result), digest_size=64).digest()
    return b"PBFT\x03" + view.to_bytes(8, "little") + ts.to_bytes(8, "little") + d


def text_of(view, ts, result, replica, pid, sig):
    """One reply's text by pbft_wire_encode_replies."""
    req = wire.pack_results([result], [ts], [b"c"])
    stream, _, _ = wire.encode_replies(view, req, replica, pid, np.frombuffer(sig, np.uint8).reshape(1, 64))
    return stream.tobytes()


def reply(w, signer, view, ts, ci, result, claim=None, pid=None, sent=None, forge=False):
    """The text replica `signer` sends for (view, ts, result) to CLIENTS[ci]; claim / pid: the "replica" and "peer_id" it
    writes (default: its own); sent: the result written into the text (default: the signed one)."""
    sig = w.sign(SEEDS[signer], envelope(view, ts, CLIENTS[ci], result))
    if forge:
        sig = bytes([sig[0] ^ 1]) + sig[1:]
    return text_of(view, ts, result if sent is None else sent, signer if claim is None else claim,
                   w.pids[signer] if pid is None else pid, sig)


def near_misses(good, pid, sig_hex):
    """tests/test_reply.py::test_near_misses_are_none, applied to `good` (view 12, timestamp 34, replica 1, result
    b"awesome!")."""
    letter = next(i for i, c in enumerate(sig_hex) if c in b"abcdef")
    upper = good.replace(sig_hex, sig_hex[:letter] + sig_hex[letter:letter + 1].upper() + sig_hex[letter + 1:])
    return {
        "a space": good.replace(b'"view":', b'"view": '),
        "another field order": good.replace(b'"view":12,"timestamp":34', b'"timestamp":34,"view":12'),
        "an escape": good.replace(b"awesome!", b"awesome\\u0021"),
        "a 51-character peer id": good.replace(pid, pid[:51]),
        "a 53-character peer id": good.replace(pid, pid + b"1"),
        "not base58": good.replace(pid, pid[:10] + b"0" + pid[11:]),
        "an uppercase hex digit": upper,
        "a trailing byte": good + b"\n",
        "a missing byte": good[:-1],
        "a leading zero": good.replace(b'"view":12', b'"view":012'),
        "a 21-digit number": good.replace(b'"view":12', b'"view":184467440737095516150'),
        "2^64": good.replace(b'"view":12', b'"view":18446744073709551616'),
        "replica 65536": good.replace(b'"replica":1', b'"replica":65536'),
        "a quote in the result": good.replace(b"awesome!", b'awe"some'),
        "empty": b"",
    }


_corpora = {}


def corpus(n_honest, salt=0, with_outside=True):
    """dict(texts, client_idx, inside, note): n_honest honest requests answered by all four replicas, then the planted
    cases, in a fixed shuffled order (the forged reply of its request moved in front of its honest siblings).
    Computed once per key and never changed."""
    key = (n_honest, salt, with_outside)
    if key in _corpora:
        return _corpora[key]
    w = world()
    rng = np.random.default_rng(9100 + salt)
    rows = []  # (text, client_idx, inside, note)

    def res(k):
        return R.ALPHABET[rng.integers(0, len(R.ALPHABET), RES_LENS[k % len(RES_LENS)])].tobytes()

    def add(note, *a, ci=0, inside=True, **kw):
        rows.append((reply(w, *a[:3], ci, *a[3:], **kw), ci, inside, note))

    ts = 1000
    for q in range(n_honest):  # the number widths of R.VALS in the first ten
        view = R.VALS[(7 * q + salt) % 10] if q < 10 else 1
        t = R.VALS[(q + salt) % 10] if q < 10 else ts + q
        r = GENERAL[q % 4] if q % 8 == 5 else res(q)
        for s in range(N_REPLICAS):
            add("honest", s, view, t, r, ci=q % 3)
    ts = 5000
    # a forged signature in front of three honest replies
    r = res(1)
    add("forged", 0, 1, ts, r, forge=True)
    for s in (1, 2, 3):
        add("forged-sibling", s, 1, ts, r)
    # one flipped result byte: replica 1's text carries another result than it signed
    r = res(2)
    for s in (0, 2):
        add("honest", s, 1, ts + 1, r, ci=1)
    add("flipped", 1, 1, ts + 1, r, ci=1, sent=r[:5] + (b"x" if r[5:6] != b"x" else b"y") + r[6:])
    # the signer's claims
    r = res(3)
    add("wrong index", 2, 1, ts + 2, r, claim=1)
    add("wrong peer id", 2, 1, ts + 2, r, pid=w.pids[3])
    add("replica 4", 0, 1, ts + 2, r, claim=4)
    add("replica 65535", 0, 1, ts + 2, r, claim=65535)
    add("honest", 3, 1, ts + 2, r)  # (alone: not accepted)
    # client_idx out of range
    rows.append((reply(w, 0, 1, ts + 3, 0, r), 3, True, "client 3"))
    rows.append((reply(w, 1, 1, ts + 3, 0, r), 2**32 - 1, True, "client 2^32 - 1"))
    # the same reply twice, and nobody else: one signer
    t0 = reply(w, 0, 1, ts + 4, 2, r)
    rows += [(t0, 2, True, "twice"), (t0, 2, True, "twice")]
    # replica 3 sends two other results for a timestamp replicas 0 and 1 answered
    r = res(4)
    for s in (0, 1):
        add("honest", s, 1, ts + 5, r)
    add("equivocation", 3, 1, ts + 5, r[:-1] + b"x")
    add("equivocation", 3, 1, ts + 5, r[:-1] + b"y")
    # the same timestamp and result to two clients, two replicas each (exactly need)
    for ci in (0, 1):
        for s in (1, 2):
            add("two clients", s, 1, ts + 6, b"awesome!", ci=ci)
    # answered by one replica, and by exactly two
    add("one answer", 2, 1, ts + 7, res(5), ci=1)
    r = res(6)
    for s in (0, 3):
        add("two answers", s, 1, ts + 8, r, ci=2)
    # general results from all four
    for k, g in enumerate(GENERAL):
        for s in range(N_REPLICAS):
            add("general", s, 1, ts + 10 + k, g, ci=k % 3)
    # the near misses, on a request two honest replicas answered; and a text cut short by one byte
    sig = w.sign(SEEDS[1], envelope(12, 34, CLIENTS[0], b"awesome!"))
    good = text_of(12, 34, b"awesome!", 1, w.pids[1], sig)
    for s in (0, 1):
        add("honest", s, 12, 34, b"awesome!")
    for name, t in near_misses(good, w.pids[1], sig.hex().encode()).items():
        rows.append((t, 0, True, "near miss: " + name))
    rows.append((reply(w, 2, 12, 34, 0, b"awesome!")[:-1], 0, True, "cut short"))
    if with_outside:  # a text that does not lie inside text_bytes (placed behind the others by pack())
        rows.append((reply(w, 3, 12, 34, 0, b"awesome!"), 0, False, "outside"))
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    notes = [r[3] for r in rows]
    fi, sib = notes.index("forged"), notes.index("forged-sibling")
    if fi > sib:
        rows[fi], rows[sib] = rows[sib], rows[fi]
    c = dict(texts=[r[0] for r in rows], client_idx=np.array([r[1] for r in rows], np.uint32),
             inside=[r[2] for r in rows], note=[r[3] for r in rows])
    _corpora[key] = c
    return c


def prefix(c, n):
    return dict(texts=c["texts"][:n], client_idx=c["client_idx"][:n].copy(), inside=c["inside"][:n], note=c["note"][:n])


def pack(c, gap=0):
    """(buffer, off, len, text_bytes): the inside texts back to back (gap bytes between them), the outside ones given
    offsets that end behind text_bytes."""
    ins = [t for t, k in zip(c["texts"], c["inside"]) if k]
    lens = np.array([len(t) for t in c["texts"]], np.uint32)
    off = np.zeros(len(lens), np.uint64)
    at, parts = 0, []
    for i, (t, k) in enumerate(zip(c["texts"], c["inside"])):
        if k:
            off[i] = at
            parts.append(t + b"\xa5" * gap)
            at += len(t) + gap
    text_bytes = at
    n_out = 0
    for i, k in enumerate(c["inside"]):
        if not k:  # the first ends a byte behind text_bytes, the others lie far outside
            off[i] = text_bytes - int(lens[i]) + 1 if n_out == 0 and text_bytes >= lens[i] else 2**40 + i
            n_out += 1
    raw = b"".join(parts)
    buf = np.full((len(raw) + 15) // 16 * 16 + 64, 0xA5, np.uint8)
    buf[:len(raw)] = np.frombuffer(raw, np.uint8)
    assert len(ins) == len(parts)
    return buf, off, lens, text_bytes


def model(c, settle, env_cap=None, pids=None, verify=None, need=NEED):
    w = world()
    n = len(c["texts"])
    return accept_reference(c["texts"], CLIENTS, w.pids if pids is None else pids, need,
                            max(n, 1) if env_cap is None else env_cap, w.verify if verify is None else verify,
                            client_idx=c["client_idx"], inside=c["inside"], settle=settle)


def records_of(m):
    """(N, 160) by pbft_records_pack from the model's rows; the zero record with key index 0xFFFF for what is not OK."""
    n = len(m["heads"])
    ok = (m["heads"]["status"] & 0xFF) == wire.ACCEPT_OK
    key = np.where(ok, m["heads"]["replica"], 0xFFFF).astype(np.uint16)
    rec = np.zeros((max(n, 1), 160), np.uint8)
    sg = np.ascontiguousarray(m["sigs"])
    R_, S_ = np.ascontiguousarray(sg[:, :32]), np.ascontiguousarray(sg[:, 32:])
    env = np.ascontiguousarray(m["env_rows"])
    if n:
        lib = wire.load()
        assert lib.pbft_records_pack(R_.ctypes.data, S_.ctypes.data, key.ctypes.data, env.ctypes.data, 85, n,
                                     rec.ctypes.data) == 0
    return rec[:n]
