"""BatchVerifier: host-side view of the GPU verifier (BASELINE.json north_star).

Mirrors the trait the reference would bind:

    trait BatchVerifier {
        fn submit(&mut self, b: &SigBatch) -> Ticket;
        fn poll(&mut self, t: Ticket) -> Option<Bitmap>;
        fn verify(&mut self, b: &SigBatch) -> Bitmap;   // blocking
    }

It replaces the per-message validators validate_prepare
(src/behavior.rs:159-175) and validate_commit (src/behavior.rs:184-195), whose
signature checks are TODOs (src/behavior.rs:127, :185).  Invalid signatures are
bit 0 in the returned bitmap, never an exception (the reference panics via
.unwrap() at src/behavior.rs:345, :371; the build drops the message instead).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from ._lib import PbftError, check, load


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data if a is not None and a.size else 0


@dataclass
class SigBatch:
    """Struct-of-arrays batch of one (view, seq) round window (or several)."""

    R: np.ndarray        # (N, 32) uint8
    S: np.ndarray        # (N, 32) uint8
    key_idx: np.ndarray  # (N,) uint16, index into the installed key set
    msg: np.ndarray      # (N, stride) uint8, first msg_len bytes signed
    msg_len: int

    def __post_init__(self):
        self.R = np.ascontiguousarray(self.R, dtype=np.uint8).reshape(-1, 32)
        self.S = np.ascontiguousarray(self.S, dtype=np.uint8).reshape(-1, 32)
        self.key_idx = np.ascontiguousarray(self.key_idx, dtype=np.uint16).reshape(-1)
        n = len(self.R)
        if len(self.S) != n or len(self.key_idx) != n:
            raise ValueError("R, S and key_idx must have the same length")
        m = np.ascontiguousarray(self.msg, dtype=np.uint8)
        if m.ndim == 1:
            m = m.reshape(n, -1) if n else m.reshape(0, max(self.msg_len, 1))
        if m.shape[0] != n or m.shape[1] < self.msg_len:
            raise ValueError("msg must be (N, stride >= msg_len)")
        self.msg = m

    def __len__(self) -> int:
        return len(self.R)


class KeyStats(ctypes.Structure):
    """pbft_key_stats (include/pbft_verify.h): phases of the last set_keys / update_keys."""
    _fields_ = [("total_ms", ctypes.c_double), ("meminfo_ms", ctypes.c_double), ("free_ms", ctypes.c_double),
                ("alloc_ms", ctypes.c_double), ("build_ms", ctypes.c_double), ("keys_built", ctypes.c_uint32),
                ("reused", ctypes.c_uint32), ("table_bytes", ctypes.c_uint64)]


class VotesStaging(ctypes.Structure):
    """pbft_votes_staging (include/pbft_verify.h)."""
    _fields_ = [("sig", ctypes.c_void_p), ("key_idx", ctypes.c_void_p), ("env_idx", ctypes.c_void_p),
                ("envelopes", ctypes.c_void_p), ("row_stride", ctypes.c_uint32)]


def bitmap_to_bool(bitmap: np.ndarray, n: int) -> np.ndarray:
    """LSB-first u64 words -> bool[n]."""
    bits = np.unpackbits(bitmap.view(np.uint8), bitorder="little")
    return bits[:n].astype(bool)


TALLY_ACCUMULATE = 1  # PBFT_TALLY_ACCUMULATE (include/pbft_verify.h)


def tally_reference(bits, key_idx, env_idx, n_env: int, n_signers: int):
    """The semantics of pbft_tally_device in numpy: (signers, counts).  signers is (n_env, W) uint64 with
    W = ceil(n_signers / 64): bit (k % 64) of signers[e, k // 64] is 1 iff some row i has bits[i] set,
    env_idx[i] == e < n_env and key_idx[i] == k < n_signers; counts[e] (uint32) is the popcount of row e, so a signer
    that votes twice under one envelope counts once and a row with either index out of range contributes nothing.
    bits: bool per row (bitmap_to_bool of the verifier's bitmap)."""
    bits = np.asarray(bits).astype(bool).reshape(-1)
    k = np.asarray(key_idx).reshape(-1).astype(np.int64)
    e = np.asarray(env_idx).reshape(-1).astype(np.int64)
    if not (len(bits) == len(k) == len(e)):
        raise ValueError("bits, key_idx and env_idx must have the same length")
    W = (n_signers + 63) // 64
    member = np.zeros((n_env, W * 64), dtype=bool)
    ok = bits & (e < n_env) & (k < n_signers)
    member[e[ok], k[ok]] = True
    signers = np.packbits(member, axis=1, bitorder="little").view(np.uint64).reshape(n_env, W)
    return signers, member.sum(axis=1).astype(np.uint32)


ENV_NONE = 0xFFFFFFFF  # env_idx of a row that pbft_group_envelopes_device skipped or that env_cap left out


def group_reference(msg_rows, skip_mask, env_cap: int):
    """The semantics of pbft_group_envelopes_device in numpy: (env_idx, envelopes, n_env).  msg_rows is (N, >= 85)
    uint8, of which the first 85 bytes of a row are its envelope; skip_mask: None or bool per row (the rows whose key
    index is 0xFFFF).  Envelope e is the e-th distinct 85-byte string in row order, by first appearance -- a dict
    filled row by row: env_idx[i] = e (uint32), envelopes (env_cap, 85) uint8 holds the first env_cap of them and
    zeros behind, n_env = [distinct envelopes found (may exceed env_cap), rows that env_cap left without an index]
    (uint32).  Skipped rows, and rows whose envelope's index is >= env_cap, get ENV_NONE."""
    rows = np.ascontiguousarray(np.asarray(msg_rows, dtype=np.uint8))
    rows = rows.reshape(len(rows), -1)[:, :85] if len(rows) else rows.reshape(0, 85)
    n = len(rows)
    skip = np.zeros(n, bool) if skip_mask is None else np.asarray(skip_mask).astype(bool).reshape(-1)
    if len(skip) != n:
        raise ValueError("skip_mask must have one entry per row")
    if n and env_cap <= 0:
        raise ValueError("env_cap must be positive")
    seen: dict = {}
    env_idx = np.full(n, ENV_NONE, dtype=np.uint32)
    envelopes = np.zeros((env_cap, 85), dtype=np.uint8)
    lost = 0
    for i in range(n):
        if skip[i]:
            continue
        e = seen.setdefault(rows[i].tobytes(), len(seen))
        if e < env_cap:
            env_idx[i] = e
            envelopes[e] = rows[i]
        else:
            lost += 1
    return env_idx, envelopes, np.array([len(seen), lost], dtype=np.uint32)


ADMIT_CLEAN, ADMIT_CONTESTED, ADMIT_REJ_VIEW, ADMIT_REJ_WATERMARK, ADMIT_REJ_SIGNER, ADMIT_HOST, ADMIT_PAD = range(7)
ADMIT_CLASSES = 8  # PBFT_ADMIT_* (include/pbft_wire.h)


def admit_reference(heads, view: int, h: int, log_window: int, n_keys: int, residue_cap: int, n_total=None,
                    off=None, flen=None) -> dict:
    """The semantics of pbft_admit_device in plain Python over a wire.FrameHead array: what the replica does with
    each decoded frame before it touches a round window.  Frame f >= min(n_total, N) is ADMIT_PAD; status ESIGNER (5)
    is ADMIT_REJ_SIGNER; any other status but OK, and kind 0, is ADMIT_HOST; an OK vote whose key index is >= n_keys
    is ADMIT_REJ_SIGNER, of another view ADMIT_REJ_VIEW (tested before the window), with seq outside (h, h +
    log_window] ADMIT_REJ_WATERMARK (integers: h + log_window may pass 2^64, the window then ends at 2^64 - 1); what
    is left is admitted, ADMIT_CONTESTED if another admitted row has its (kind, seq, signer), else ADMIT_CLEAN.
    Returns cls (N,) uint8, counts (8,) uint32, clean (ceil(N / 64),) uint64 bitmap, res (residue_cap,) wire.AdmitResidue
    = the CONTESTED and HOST frames in frame order (zeros behind; off / len from `off` / `flen`, 0 without them),
    n_res (2,) uint32 = [their number, those residue_cap left out], and keep (N,) bool = the rows whose record keeps
    its key index (the others get 0xFFFF)."""
    from .wire import AdmitResidue
    n = len(heads)
    n_valid = n if n_total is None else min(int(n_total), n)
    cls = np.zeros(n, dtype=np.uint8)
    seen: dict = {}
    for f in range(n):
        hd = heads[f]
        st, kind, key = int(hd["status"]), int(hd["kind"]), int(hd["key_idx"])
        if f >= n_valid:
            c = ADMIT_PAD
        elif st == 5:
            c = ADMIT_REJ_SIGNER
        elif st != 0 or kind not in (1, 2):
            c = ADMIT_HOST
        elif key >= n_keys:
            c = ADMIT_REJ_SIGNER
        elif int(hd["view"]) != view:
            c = ADMIT_REJ_VIEW
        elif not (h < int(hd["seq"]) <= h + log_window):
            c = ADMIT_REJ_WATERMARK
        else:
            c = ADMIT_CLEAN
            seen.setdefault((kind, int(hd["seq"]), key), []).append(f)
        cls[f] = c
    for rows in seen.values():
        if len(rows) > 1:
            cls[rows] = ADMIT_CONTESTED
    counts = np.bincount(cls, minlength=ADMIT_CLASSES).astype(np.uint32)
    keep = cls == ADMIT_CLEAN
    bits = np.zeros((n + 63) // 64 * 64, dtype=np.uint8)
    bits[:n] = keep
    clean = np.packbits(bits, bitorder="little").view(np.uint64) if n else np.zeros(0, np.uint64)
    res = np.zeros(residue_cap, dtype=AdmitResidue)
    frames = np.flatnonzero((cls == ADMIT_CONTESTED) | (cls == ADMIT_HOST))
    for at, f in enumerate(frames[:residue_cap]):
        res[at] = (0 if off is None else int(off[f]), f, 0 if flen is None else int(flen[f]))
    n_res = np.array([len(frames), max(0, len(frames) - residue_cap)], dtype=np.uint32)
    return dict(cls=cls, counts=counts, clean=clean, res=res, n_res=n_res, keep=keep)


_B58_SET = frozenset(b"123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz")
_U64 = rb"(0|[1-9][0-9]{0,19})"
_CANONICAL_REPLY = None


def _canonical_reply(text: bytes):
    """The canonical signed reply (reply_core.h's rp_match) as a regular expression: (view, timestamp, peer_id, result
    span, replica, signature bytes) or None."""
    import re
    global _CANONICAL_REPLY
    if _CANONICAL_REPLY is None:
        _CANONICAL_REPLY = re.compile(
            rb'\{"view":' + _U64 + rb',"timestamp":' + _U64 +
            rb',"peer_id":"([1-9A-HJ-NP-Za-km-z]{52})","result":"([ !#-\[\]-~]{0,3072})","replica":(0|[1-9][0-9]{0,4})'
            rb',"signature":"([0-9a-f]{128})"\}')
    m = _CANONICAL_REPLY.fullmatch(text)
    if not m:
        return None
    view, ts, rep = int(m.group(1)), int(m.group(2)), int(m.group(5))
    if view >= 2**64 or ts >= 2**64 or rep > 65535:
        return None
    return view, ts, m.group(3), m.span(4), rep, bytes.fromhex(m.group(6).decode())


def _json_reply(text: bytes):
    """A signed ClientReply by serde's rules, with `json`: (view, timestamp, peer_id, raw span of the result, replica,
    signature bytes, result bytes) or None.  (A model for texts a serializer wrote and their variants: it does not
    chase the corners where Python's reader is laxer than serde's inside unknown fields, such as NaN.)"""
    import json
    try:
        s = text.decode("utf-8")

        def pairs(p):
            d = dict(p)
            if len(d) != len(p):
                raise ValueError("duplicate field")
            return d
        j = json.loads(s, object_pairs_hook=pairs)
    except (ValueError, RecursionError):
        return None
    if not isinstance(j, dict) or not {"view", "timestamp", "peer_id", "result", "replica", "signature"} <= set(j):
        return None
    for k, top in (("view", 2**64), ("timestamp", 2**64), ("replica", 65536)):
        if type(j[k]) is not int or not 0 <= j[k] < top:
            return None
    if not all(isinstance(j[k], str) for k in ("peer_id", "result", "signature")):
        return None
    try:
        pid, sig, res = j["peer_id"].encode(), j["signature"].encode(), j["result"].encode("utf-8")
    except UnicodeEncodeError:  # a lone surrogate escape
        return None
    if len(pid) != 52 or not set(pid) <= _B58_SET or len(sig) != 128 or not set(sig) <= set(b"0123456789abcdef"):
        return None
    # the raw span of the top-level "result": walk the object's members
    b, i, span = text, text.index(b"{") + 1, None

    def string_end(i):  # i at the opening quote -> the index behind the closing one
        i += 1
        while b[i] != 0x22:
            i += 2 if b[i] == 0x5C else 1
        return i + 1
    while True:
        while b[i] in b" \t\n\r,":
            i += 1
        if b[i] == 0x7D:
            break
        k0, i = i, string_end(i)
        key = json.loads(b[k0:i].decode())
        while b[i] in b" \t\n\r:":
            i += 1
        if b[i] == 0x22:
            v0, i = i, string_end(i)
            if key == "result":
                span = (v0 + 1, i - 1)
        else:
            depth = 0
            while True:
                if b[i] == 0x22:
                    i = string_end(i)
                    continue
                if b[i] in b"{[":
                    depth += 1
                elif b[i] in b"}]":
                    if depth == 0:
                        break
                    depth -= 1
                elif b[i] == 0x2C and depth == 0:
                    break
                i += 1
    return j["view"], j["timestamp"], pid, span, j["replica"], bytes.fromhex(sig.decode()), res


def accept_reference(texts, clients, peer_ids, need: int, env_cap: int, verify, client_idx=None, inside=None,
                     settle: bool = True) -> dict:
    """The client's acceptance rule (include/pbft_wire.h, pbft_accept_replies) in plain Python, the tests' model.
    texts: the replies (bytes each); clients: the client address fields (bytes or str, as wire.client_field takes them);
    peer_ids: the 52-character PeerId text of every installed key, by key index; client_idx: None or one index into
    `clients` per reply; inside: None or a bool per reply (False: the text does not lie inside text_bytes);
    verify(replica, sig64, envelope85) -> bool answers for one signature.  settle=True is the blocking form (a text that
    is not canonical goes through `json`: EJSON or settled), False the device form (such a text is EDEFER).
    Returns a dict: heads (wire.AcceptHead), sigs (N, 64), env_rows (N, 85; zero unless OK), bits (N,) bool, env_idx,
    envelopes (env_cap, 85), n_env (2,), signers (env_cap, W) uint64, counts, certs (wire.AcceptCert), results (the
    result bytes of every OK reply, else None)."""
    import hashlib

    from .wire import (ACCEPT_ECLIENT, ACCEPT_EDEFER, ACCEPT_EJSON, ACCEPT_ESCAPED, ACCEPT_ESIGNER, ACCEPT_NO_REPLY,
                       ACCEPT_OK, AcceptCert, AcceptHead, client_field)
    n, n_keys = len(texts), len(peer_ids)
    heads = np.zeros(n, AcceptHead)
    sigs, env_rows = np.zeros((n, 64), np.uint8), np.zeros((n, 85), np.uint8)
    results = [None] * n
    for i, t in enumerate(texts):
        t = bytes(t)
        heads[i]["status"] = ACCEPT_EDEFER
        if inside is not None and not inside[i]:
            continue
        flag = 0
        c = _canonical_reply(t)
        if c is not None:
            view, ts, pid, span, rep, sig = c
            res = t[span[0]:span[1]]
        elif not settle:
            continue
        else:
            g = _json_reply(t)
            if g is None:
                heads[i]["status"] = ACCEPT_EJSON
                continue
            view, ts, pid, span, rep, sig, res = g
            flag = ACCEPT_ESCAPED if b"\\" in t[span[0]:span[1]] else 0
        if rep >= n_keys or bytes(peer_ids[rep]) != pid:
            heads[i]["status"] = ACCEPT_ESIGNER
            continue
        ci = 0 if client_idx is None else int(client_idx[i])
        if ci >= len(clients):
            heads[i]["status"] = ACCEPT_ECLIENT
            continue
        heads[i] = (view, ts, span[0], span[1] - span[0], rep, ACCEPT_OK | flag)
        d = hashlib.blake2b(client_field(clients[ci]) + res, digest_size=64).digest()
        env = b"PBFT\x03" + view.to_bytes(8, "little") + ts.to_bytes(8, "little") + d
        sigs[i], env_rows[i] = np.frombuffer(sig, np.uint8), np.frombuffer(env, np.uint8)
        results[i] = res
    ok = (heads["status"] & 0xFF) == ACCEPT_OK
    seen: dict = {}
    env_idx = np.full(n, ENV_NONE, np.uint32)
    envelopes = np.zeros((env_cap, 85), np.uint8)
    lost = 0
    bits = np.zeros(n, bool)
    W = (n_keys + 63) // 64
    sets = [set() for _ in range(env_cap)]
    first = [ACCEPT_NO_REPLY] * env_cap
    for i in range(n):
        if not ok[i]:
            continue
        rep = int(heads[i]["replica"])
        bits[i] = bool(verify(rep, sigs[i].tobytes(), env_rows[i].tobytes()))
        e = seen.setdefault(env_rows[i].tobytes(), len(seen))
        if e >= env_cap:
            lost += 1
            continue
        env_idx[i], envelopes[e] = e, env_rows[i]
        if bits[i]:
            sets[e].add(rep)
            first[e] = min(first[e], i)
    signers = np.zeros((env_cap, W), np.uint64)
    counts = np.zeros(env_cap, np.uint32)
    certs = np.zeros(env_cap, AcceptCert)
    certs["first"] = ACCEPT_NO_REPLY
    for e in range(min(len(seen), env_cap)):
        for r in sets[e]:
            signers[e, r // 64] |= np.uint64(1 << (r % 64))
        counts[e] = len(sets[e])
        cl = 0 if first[e] == ACCEPT_NO_REPLY or client_idx is None else int(client_idx[first[e]])
        env = envelopes[e].tobytes()
        certs[e] = (int.from_bytes(env[5:13], "little"), int.from_bytes(env[13:21], "little"), first[e], len(sets[e]), cl,
                    int(len(sets[e]) >= need))
    return dict(heads=heads, sigs=sigs, env_rows=env_rows, bits=bits, env_idx=env_idx, envelopes=envelopes,
                n_env=np.array([len(seen), lost], np.uint32), signers=signers, counts=counts, certs=certs,
                results=results)


def quorum(counts, need: int) -> np.ndarray:
    """Envelopes with at least `need` distinct valid signers (2f for prepared, 2f + 1 for committed-local:
    src/behavior.rs:177-182, :214-223); bool per envelope."""
    return np.asarray(counts) >= need


def verify_multi(verifiers, b: "SigBatch") -> np.ndarray:
    """pbft_verify_batch_multi: shard one batch over several contexts (GPUs and/or clones); bitmap words."""
    lib = load()
    n = len(b)
    out = np.zeros((n + 63) // 64, dtype=np.uint64)
    arr = (ctypes.c_void_p * len(verifiers))(*[v._ctx.value for v in verifiers])
    check(lib.pbft_verify_batch_multi(arr, len(verifiers), _ptr(b.R), _ptr(b.S), _ptr(b.key_idx), _ptr(b.msg),
                                      b.msg_len, b.msg.shape[1], n, _ptr(out)))
    return out


class MultiGpu:
    """pbft_multi_create / pbft_verify_batch_device_multi: one context per device of this process, the round's
    bitmap words all-gathered on RCCL (include/pbft_verify.h)."""

    def __init__(self, verifiers):
        self._lib = load()
        self._m = ctypes.c_void_p()
        # the contexts must outlive the communicator (destroy synchronises their streams): hold the verifiers
        self._verifiers = list(verifiers)
        arr = (ctypes.c_void_p * len(verifiers))(*[v._ctx.value for v in verifiers])
        check(self._lib.pbft_multi_create(arr, len(verifiers), ctypes.byref(self._m)))
        self.n = len(verifiers)

    def verify_device(self, d_R, d_S, d_K, d_M, n, words_per_rank, d_bitmaps, msg_len=85, msg_stride=85):
        """Per-rank lists of device pointers / counts; enqueue only (sync() to wait)."""
        P = ctypes.c_void_p * self.n
        check(self._lib.pbft_verify_batch_device_multi(self._m, P(*d_R), P(*d_S), P(*d_K), P(*d_M), msg_len,
                                                       msg_stride, (ctypes.c_uint64 * self.n)(*n), words_per_rank,
                                                       P(*d_bitmaps)))

    def sync(self):
        check(self._lib.pbft_multi_sync(self._m))

    def close(self):
        if self._m:
            self._lib.pbft_multi_destroy(self._m)
            self._m = ctypes.c_void_p()
        self._verifiers = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GpuBatchVerifier:
    """One HIP context (one GPU).  Not thread-safe: one per host thread."""

    def __init__(self, device: int = 0, _parent: "GpuBatchVerifier | None" = None):
        self._lib = load()
        self._ctx = ctypes.c_void_p()
        if _parent is None:
            check(self._lib.pbft_verify_ctx_create(device, ctypes.byref(self._ctx)))
            self.n_keys = 0
        else:
            check(self._lib.pbft_verify_ctx_clone(_parent._ctx, ctypes.byref(self._ctx)))
            device, self.n_keys = _parent.device, _parent.n_keys
        self.device = device
        self._pending = None

    def clone(self) -> "GpuBatchVerifier":
        """Another context (own HIP stream and workspace) sharing this one's tables and key set."""
        return GpuBatchVerifier(_parent=self)

    # -- key set (libp2p identity keys, src/main.rs:39-40) ------------------
    def set_keys(self, keys: np.ndarray) -> np.ndarray:
        keys = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1, 32)
        ok = np.zeros(len(keys), dtype=np.uint8)
        check(self._lib.pbft_verify_set_keys(self._ctx, _ptr(keys), len(keys), _ptr(ok)))
        self.n_keys = len(keys)
        return ok.astype(bool)

    def update_keys(self, idx, keys: np.ndarray) -> np.ndarray:
        """pbft_verify_update_keys: key idx[i] of the installed set becomes keys[i] (only those tables rebuilt);
        returns key_ok of the new keys."""
        idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
        keys = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1, 32)
        if len(idx) != len(keys):
            raise ValueError("idx and keys must have the same length")
        ok = np.zeros(len(keys), dtype=np.uint8)
        check(self._lib.pbft_verify_update_keys(self._ctx, _ptr(idx), _ptr(keys), len(keys), _ptr(ok)))
        return ok.astype(bool)

    def key_stats(self) -> dict:
        """Phases of the last set_keys / update_keys (ms), keys built, whether the allocation was reused."""
        st = KeyStats()
        check(self._lib.pbft_verify_key_stats(self._ctx, ctypes.byref(st)))
        return {k: getattr(st, k) for k, _ in KeyStats._fields_}

    # -- BatchVerifier -------------------------------------------------------
    def verify(self, b: SigBatch) -> np.ndarray:
        """Blocking; returns the ceil(N/64) u64 bitmap words."""
        n = len(b)
        out = np.zeros((n + 63) // 64, dtype=np.uint64)
        check(self._lib.pbft_verify_batch(self._ctx, _ptr(b.R), _ptr(b.S), _ptr(b.key_idx), _ptr(b.msg),
                                          b.msg_len, b.msg.shape[1], n, _ptr(out)))
        return out

    def submit(self, b: SigBatch) -> int:
        n = len(b)
        out = np.zeros((n + 63) // 64, dtype=np.uint64)
        check(self._lib.pbft_verify_batch_async(self._ctx, _ptr(b.R), _ptr(b.S), _ptr(b.key_idx), _ptr(b.msg),
                                                b.msg_len, b.msg.shape[1], n, _ptr(out)))
        self._pending = (b, out)  # keep host buffers alive until poll/wait
        return id(out)

    def poll(self, ticket: int):
        if self._pending is None or id(self._pending[1]) != ticket:
            raise PbftError(-1, "unknown ticket")
        if check(self._lib.pbft_verify_poll(self._ctx)) == 1:
            out = self._pending[1]
            self._pending = None
            return out
        return None

    def wait(self, ticket: int) -> np.ndarray:
        if self._pending is None or id(self._pending[1]) != ticket:
            raise PbftError(-1, "unknown ticket")
        check(self._lib.pbft_verify_wait(self._ctx))
        out = self._pending[1]
        self._pending = None
        return out

    def verify_device(self, d_R: int, d_S: int, d_key_idx: int, d_msg: int, msg_len: int, msg_stride: int,
                      n: int, d_bitmap: int, stream: int = 0) -> None:
        """Enqueue on device-resident buffers (raw device pointers)."""
        check(self._lib.pbft_verify_batch_device(self._ctx, d_R, d_S, d_key_idx, d_msg, msg_len, msg_stride, n,
                                                 d_bitmap, stream or None))

    def verify_device_pipelined(self, d_R: int, d_S: int, d_key_idx: int, d_msg: int, msg_len: int,
                                msg_stride: int, n: int, d_bitmap: int, stream: int, finish_stream: int) -> None:
        """Kernel on `stream`, finish (bitmap) on `finish_stream`: the next call's kernel overlaps this finish."""
        check(self._lib.pbft_verify_batch_device_pipelined(self._ctx, d_R, d_S, d_key_idx, d_msg, msg_len, msg_stride,
                                                           n, d_bitmap, stream, finish_stream))

    def reserve(self, max_n: int) -> None:
        """Pre-size the workspace (required before capturing verify_device into a graph)."""
        check(self._lib.pbft_verify_reserve(self._ctx, max_n))

    # -- uninstalled keys: the public key travels with the signature --------
    def verify_keys(self, R, S, A, msg, msg_len: int) -> np.ndarray:
        """pbft_verify_batch_keys: signature i under the key A[i] (32 raw bytes), no key set needed.  Blocking;
        returns the ceil(N/64) u64 bitmap words."""
        R = np.ascontiguousarray(R, np.uint8).reshape(-1, 32)
        S = np.ascontiguousarray(S, np.uint8).reshape(-1, 32)
        A = np.ascontiguousarray(A, np.uint8).reshape(-1, 32)
        n = len(R)
        if len(S) != n or len(A) != n:
            raise ValueError("R, S and A must have the same length")
        m = np.ascontiguousarray(msg, np.uint8)
        if m.ndim == 1:
            m = m.reshape(n, -1) if n else m.reshape(0, max(msg_len, 1))
        if m.shape[0] != n or m.shape[1] < msg_len:
            raise ValueError("msg must be (N, stride >= msg_len)")
        out = np.zeros((n + 63) // 64, dtype=np.uint64)
        check(self._lib.pbft_verify_batch_keys(self._ctx, _ptr(R), _ptr(S), _ptr(A), _ptr(m), msg_len, m.shape[1], n,
                                               _ptr(out)))
        return out

    def verify_keys_device(self, d_R: int, d_S: int, d_A: int, d_msg: int, msg_len: int, msg_stride: int, n: int,
                           d_bitmap: int, stream: int = 0) -> None:
        """pbft_verify_batch_keys_device: enqueue on device-resident buffers (raw device pointers)."""
        check(self._lib.pbft_verify_batch_keys_device(self._ctx, d_R, d_S, d_A, d_msg, msg_len, msg_stride, n,
                                                      d_bitmap, stream or None))

    def debug_anykey_point(self, s, k, A):
        """Test hook: (encodings (n, 32), key_ok (n,)) of [s]B + [k](-A) for n triples of 32-byte rows."""
        s = np.ascontiguousarray(s, np.uint8).reshape(-1, 32)
        k = np.ascontiguousarray(k, np.uint8).reshape(-1, 32)
        A = np.ascontiguousarray(A, np.uint8).reshape(-1, 32)
        n = len(s)
        enc, ok = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
        check(self._lib.pbft_debug_anykey_point(self._ctx, _ptr(s), _ptr(k), _ptr(A), n, _ptr(enc), _ptr(ok)))
        return enc, ok

    def verify_votes(self, R, S, key_idx, env_idx, envelopes) -> np.ndarray:
        """pbft_verify_votes: signature i signs envelopes[env_idx[i]] (85 B each); returns bitmap words."""
        R = np.ascontiguousarray(R, np.uint8).reshape(-1, 32)
        S = np.ascontiguousarray(S, np.uint8).reshape(-1, 32)
        K = np.ascontiguousarray(key_idx, np.uint16).reshape(-1)
        I = np.ascontiguousarray(env_idx, np.uint32).reshape(-1)
        E = np.ascontiguousarray(envelopes, np.uint8).reshape(-1, 85)
        n = len(R)
        if not (len(S) == len(K) == len(I) == n):
            raise ValueError("R, S, key_idx, env_idx must have the same length")
        out = np.zeros((n + 63) // 64, dtype=np.uint64)
        check(self._lib.pbft_verify_votes(self._ctx, _ptr(R), _ptr(S), _ptr(K), _ptr(I), _ptr(E), len(E), n, _ptr(out)))
        return out

    def submit_votes(self, R, S, key_idx, env_idx, envelopes) -> int:
        """pbft_verify_votes_async: non-blocking votes form; complete with poll / wait (the library copies
        pageable buffers into its pinned staging, so the arrays may be reused once this returns)."""
        R = np.ascontiguousarray(R, np.uint8).reshape(-1, 32)
        S = np.ascontiguousarray(S, np.uint8).reshape(-1, 32)
        K = np.ascontiguousarray(key_idx, np.uint16).reshape(-1)
        I = np.ascontiguousarray(env_idx, np.uint32).reshape(-1)
        E = np.ascontiguousarray(envelopes, np.uint8).reshape(-1, 85)
        n = len(R)
        if not (len(S) == len(K) == len(I) == n):
            raise ValueError("R, S, key_idx, env_idx must have the same length")
        out = np.zeros((n + 63) // 64, dtype=np.uint64)
        check(self._lib.pbft_verify_votes_async(self._ctx, _ptr(R), _ptr(S), _ptr(K), _ptr(I), _ptr(E), len(E), n,
                                                _ptr(out)))
        self._pending = ((R, S, K, I, E), out)  # (pinned inputs are DMA'd in place: keep them alive)
        return id(out)

    def stage_votes(self, n: int, n_env: int) -> dict:
        """pbft_verify_votes_stage: numpy views of the context's pinned staging for an (n, n_env) votes batch
        (72-byte rows: sig R || S, key_idx, env_idx as strided views of them; envelopes), to be filled in place and
        launched by submit_staged.
        The views are valid only until the next call on this context that uses the staging (another stage_votes,
        or any host-buffer submit / verify): do not touch them afterwards."""
        st = VotesStaging()
        check(self._lib.pbft_verify_votes_stage(self._ctx, n, n_env, ctypes.byref(st)))

        def view(ptr, dtype, shape):
            count = int(np.prod(shape))
            if count == 0:
                return np.zeros(shape, dtype)
            buf = (ctypes.c_uint8 * (count * np.dtype(dtype).itemsize)).from_address(ptr)
            return np.frombuffer(buf, dtype=dtype).reshape(shape)
        # the rows (PBFT_VOTES_ROW_BYTES each: signature, key_idx at 64, env_idx at 68) as one byte array, the
        # three fields as strided views of it
        rs = int(st.row_stride)
        rows = view(st.sig, np.uint8, (n, rs))
        return {"sig": rows[:, :64], "key_idx": rows[:, 64:66].view(np.uint16).reshape(n),
                "env_idx": rows[:, 68:72].view(np.uint32).reshape(n), "rows": rows,
                "envelopes": view(st.envelopes, np.uint8, (n_env, 85))}

    def submit_staged(self, n: int, n_env: int) -> int:
        out = np.zeros((n + 63) // 64, dtype=np.uint64)
        check(self._lib.pbft_verify_votes_submit(self._ctx, n, n_env, _ptr(out)))
        self._pending = (None, out)
        return id(out)

    def verify_votes_device(self, d_R: int, d_S: int, d_key_idx: int, d_env_idx: int, d_envelopes: int,
                            n_env: int, n: int, d_bitmap: int, stream: int = 0) -> None:
        check(self._lib.pbft_verify_votes_device(self._ctx, d_R, d_S, d_key_idx, d_env_idx, d_envelopes, n_env, n,
                                                 d_bitmap, stream or None))

    def tally_device(self, d_bitmap: int, d_key_idx: int, d_env_idx: int, n: int, n_env: int, n_signers: int,
                     d_signers: int, d_count: int, stream: int = 0, key_stride: int = 2, env_stride: int = 4,
                     flags: int = 0) -> None:
        """pbft_tally_device: enqueue the tally of n rows (raw device pointers; d_signers is [n_env][W] u64 with
        W = ceil(n_signers / 64), d_count [n_env] u32) on `stream`, behind the launch that wrote d_bitmap.
        flags = TALLY_ACCUMULATE ORs into the sets already there."""
        check(self._lib.pbft_tally_device(self._ctx, d_bitmap or None, d_key_idx or None, key_stride,
                                          d_env_idx or None, env_stride, n, n_env, n_signers, flags,
                                          d_signers or None, d_count or None, stream or None))

    def verify_votes_tally(self, R, S, key_idx, env_idx, envelopes):
        """pbft_verify_votes_tally: verify_votes and the tally of its result over the installed keys; returns
        (bitmap words, signers (n_env, W) uint64, counts (n_env,) uint32)."""
        R = np.ascontiguousarray(R, np.uint8).reshape(-1, 32)
        S = np.ascontiguousarray(S, np.uint8).reshape(-1, 32)
        K = np.ascontiguousarray(key_idx, np.uint16).reshape(-1)
        I = np.ascontiguousarray(env_idx, np.uint32).reshape(-1)
        E = np.ascontiguousarray(envelopes, np.uint8).reshape(-1, 85)
        n = len(R)
        if not (len(S) == len(K) == len(I) == n):
            raise ValueError("R, S, key_idx, env_idx must have the same length")
        out = np.zeros((n + 63) // 64, dtype=np.uint64)
        signers = np.zeros((len(E), (self.n_keys + 63) // 64), dtype=np.uint64)
        counts = np.zeros(len(E), dtype=np.uint32)
        check(self._lib.pbft_verify_votes_tally(self._ctx, _ptr(R), _ptr(S), _ptr(K), _ptr(I), _ptr(E), len(E), n,
                                                _ptr(out), _ptr(signers), _ptr(counts)))
        return out, signers, counts

    def verify_records(self, records: np.ndarray) -> np.ndarray:
        """Blocking verify of (N, 160) binary wire records (include/pbft_wire.h); returns bitmap words."""
        rec = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, 160)
        n = len(rec)
        out = np.zeros((n + 63) // 64, dtype=np.uint64)
        check(self._lib.pbft_verify_records(self._ctx, _ptr(rec), n, _ptr(out)))
        return out

    def verify_frames(self, stream, off, flen, peer=None, n_replicas: int | None = None):
        """pbft_verify_frames: the JSON frames stream[off[f] : off[f] + flen[f]] (wire.frame_index) decoded on the GPU
        -- what is not a canonical signed vote by the host's parser -- and verified.  peer: None or the authenticated
        replica index of each frame's connection; n_replicas defaults to the installed key count.  Returns (bitmap
        words, heads as a wire.FrameHead array, records (N, 160) uint8); heads["status"] is what
        wire.decode_votes gives (plus the peer rule), bit f is set iff frame f is OK and its signature verifies."""
        from .wire import FrameHead
        buf = np.ascontiguousarray(np.frombuffer(stream, np.uint8) if isinstance(stream, (bytes, bytearray))
                                   else stream, np.uint8).reshape(-1)
        off = np.ascontiguousarray(off, np.uint64).reshape(-1)
        flen = np.ascontiguousarray(flen, np.uint32).reshape(-1)
        n = len(off)
        if len(flen) != n:
            raise ValueError("off and flen must have the same length")
        if peer is not None:
            peer = np.ascontiguousarray(peer, np.uint16).reshape(-1)
            if len(peer) != n:
                raise ValueError("peer must have one entry per frame")
        out = np.zeros((n + 63) // 64, dtype=np.uint64)
        heads = np.zeros(n, dtype=FrameHead)
        records = np.zeros((n, 160), dtype=np.uint8)
        check(self._lib.pbft_verify_frames(self._ctx, _ptr(buf), len(buf), _ptr(off), _ptr(flen),
                                           _ptr(peer) if peer is not None else None,
                                           self.n_keys if n_replicas is None else n_replicas, n, _ptr(out),
                                           _ptr(heads), _ptr(records)))
        return out, heads, records

    def decode_frames_device(self, d_stream: int, stream_bytes: int, d_off: int, d_len: int, n_replicas: int, n: int,
                             d_records: int, d_heads: int, d_peer: int = 0, stream: int = 0) -> None:
        """pbft_wire_decode_frames_device: enqueue the decode of n frames (raw device pointers; d_stream 16-byte
        aligned and readable up to stream_bytes rounded up to 16) into d_records (n x 160 B) and d_heads (n x 24 B).
        Frames that are not canonical signed votes are marked wire.EDEFER."""
        check(self._lib.pbft_wire_decode_frames_device(self._ctx, d_stream or None, stream_bytes, d_off or None,
                                                       d_len or None, d_peer or None, n_replicas, n,
                                                       d_records or None, d_heads or None, stream or None))

    def verify_frames_device(self, d_stream: int, stream_bytes: int, d_off: int, d_len: int, n_replicas: int, n: int,
                             d_records: int, d_heads: int, d_bitmap: int, d_peer: int = 0, stream: int = 0) -> None:
        """pbft_verify_frames_device: decode_frames_device, then the verify of d_records on the same stream (reserve(n)
        before capturing it into a graph)."""
        check(self._lib.pbft_verify_frames_device(self._ctx, d_stream or None, stream_bytes, d_off or None,
                                                  d_len or None, d_peer or None, n_replicas, n, d_records or None,
                                                  d_heads or None, d_bitmap or None, stream or None))

    def group_reserve(self, max_n: int) -> None:
        """pbft_group_reserve: pre-size the grouping workspace (required before capturing group_envelopes_device or
        verify_frames_tally_device into a graph)."""
        check(self._lib.pbft_group_reserve(self._ctx, max_n))

    def group_envelopes_device(self, d_msg: int, n: int, env_cap: int, d_env_idx: int, d_envelopes: int,
                               d_n_env: int, msg_stride: int = 85, d_key_idx: int = 0, key_stride: int = 2,
                               stream: int = 0) -> None:
        """pbft_group_envelopes_device: enqueue the grouping of n rows (raw device pointers; row i's envelope at
        d_msg + i * msg_stride; d_key_idx 0 or a u16 per row with stride key_stride, 0xFFFF = skip the row) into
        d_env_idx [n] u32, d_envelopes [env_cap][85] and d_n_env [2] u32 -- see group_reference."""
        check(self._lib.pbft_group_envelopes_device(self._ctx, d_msg or None, msg_stride, d_key_idx or None,
                                                    key_stride, n, env_cap, d_env_idx or None, d_envelopes or None,
                                                    d_n_env or None, stream or None))

    def verify_frames_tally_device(self, d_stream: int, stream_bytes: int, d_off: int, d_len: int, n_replicas: int,
                                   n: int, d_records: int, d_heads: int, d_bitmap: int, env_cap: int, d_env_idx: int,
                                   d_envelopes: int, d_n_env: int, d_signers: int, d_count: int, d_peer: int = 0,
                                   stream: int = 0) -> None:
        """pbft_verify_frames_tally_device: decode, group, verify and tally of n frames on one stream (reserve(n) and
        group_reserve(n) before capturing it into a graph)."""
        check(self._lib.pbft_verify_frames_tally_device(
            self._ctx, d_stream or None, stream_bytes, d_off or None, d_len or None, d_peer or None, n_replicas, n,
            d_records or None, d_heads or None, d_bitmap or None, env_cap, d_env_idx or None, d_envelopes or None,
            d_n_env or None, d_signers or None, d_count or None, stream or None))

    def verify_frames_tally(self, stream, off, flen, env_cap: int, peer=None, n_replicas: int | None = None,
                            want_env_idx: bool = True):
        """pbft_verify_frames_tally: verify_frames, with the frames grouped by envelope and tallied on the GPU.
        Returns (bitmap words, heads, env_idx (N,) uint32 or None, envelopes (env_cap, 85) uint8, n_env (2,) uint32,
        signers (env_cap, W) uint64, counts (env_cap,) uint32): quorum(counts, 2 * f) answers Pbft::prepared for
        every envelope at once."""
        from .wire import FrameHead
        buf = np.ascontiguousarray(np.frombuffer(stream, np.uint8) if isinstance(stream, (bytes, bytearray))
                                   else stream, np.uint8).reshape(-1)
        off = np.ascontiguousarray(off, np.uint64).reshape(-1)
        flen = np.ascontiguousarray(flen, np.uint32).reshape(-1)
        n = len(off)
        if len(flen) != n:
            raise ValueError("off and flen must have the same length")
        if peer is not None:
            peer = np.ascontiguousarray(peer, np.uint16).reshape(-1)
            if len(peer) != n:
                raise ValueError("peer must have one entry per frame")
        out = np.zeros((n + 63) // 64, dtype=np.uint64)
        heads = np.zeros(n, dtype=FrameHead)
        env_idx = np.zeros(n, dtype=np.uint32) if want_env_idx else None
        envelopes = np.zeros((env_cap, 85), dtype=np.uint8)
        n_env = np.zeros(2, dtype=np.uint32)
        signers = np.zeros((env_cap, (self.n_keys + 63) // 64), dtype=np.uint64)
        counts = np.zeros(env_cap, dtype=np.uint32)
        check(self._lib.pbft_verify_frames_tally(
            self._ctx, _ptr(buf), len(buf), _ptr(off), _ptr(flen), _ptr(peer) if peer is not None else None,
            self.n_keys if n_replicas is None else n_replicas, n, env_cap, _ptr(out), _ptr(heads),
            _ptr(env_idx) if want_env_idx else None, _ptr(envelopes), n_env.ctypes.data, _ptr(signers),
            _ptr(counts)))
        return out, heads, env_idx, envelopes, n_env, signers, counts

    def index_reserve(self, max_stream_bytes: int, max_segments: int) -> None:
        """pbft_index_reserve: pre-size the index workspace at the current OPT_INDEX_TILE (required before capturing
        index_streams_device or verify_streams_tally_device into a graph)."""
        check(self._lib.pbft_index_reserve(self._ctx, max_stream_bytes, max_segments))

    def index_streams_device(self, d_stream: int, stream_bytes: int, d_seg_off: int, d_seg_len: int, n_segments: int,
                             frame_cap: int, d_off: int, d_len: int, d_seg_heads: int, d_n_frames: int,
                             d_seg_peer: int = 0, d_peer: int = 0, stream: int = 0) -> None:
        """pbft_wire_index_streams_device: enqueue the frame index of n_segments connection segments of one stream (raw
        device pointers): d_off / d_len / d_peer [frame_cap], d_seg_heads [n_segments] (wire.SegHead), d_n_frames [2]
        u32 = (total, not written)."""
        check(self._lib.pbft_wire_index_streams_device(
            self._ctx, d_stream or None, stream_bytes, d_seg_off or None, d_seg_len or None, d_seg_peer or None,
            n_segments, frame_cap, d_off or None, d_len or None, d_peer or None, d_seg_heads or None,
            d_n_frames or None, stream or None))

    def verify_streams_tally_device(self, d_stream: int, stream_bytes: int, d_seg_off: int, d_seg_len: int,
                                    n_segments: int, n_replicas: int, frame_cap: int, d_off: int, d_len: int,
                                    d_seg_heads: int, d_n_frames: int, d_records: int, d_heads: int, d_bitmap: int,
                                    env_cap: int, d_env_idx: int, d_envelopes: int, d_n_env: int, d_signers: int,
                                    d_count: int, d_seg_peer: int = 0, d_peer: int = 0, stream: int = 0) -> None:
        """pbft_verify_streams_tally_device: index_streams_device, then verify_frames_tally_device with n = frame_cap
        on the same stream (reserve(frame_cap), group_reserve(frame_cap) and index_reserve before a capture)."""
        check(self._lib.pbft_verify_streams_tally_device(
            self._ctx, d_stream or None, stream_bytes, d_seg_off or None, d_seg_len or None, d_seg_peer or None,
            n_segments, n_replicas, frame_cap, d_off or None, d_len or None, d_peer or None, d_seg_heads or None,
            d_n_frames or None, d_records or None, d_heads or None, d_bitmap or None, env_cap, d_env_idx or None,
            d_envelopes or None, d_n_env or None, d_signers or None, d_count or None, stream or None))

    def verify_streams_tally(self, stream, seg_off, seg_len, frame_cap: int, env_cap: int, seg_peer=None,
                             n_replicas: int | None = None, want_index: bool = False):
        """pbft_verify_streams_tally: verify_frames_tally of per-connection segments of `stream`, the frame index made
        on the GPU.  seg_peer: None or the authenticated replica index of each segment's connection.  Returns a dict:
        n (frames verified = min(total, frame_cap)), bitmap, heads, env_idx, envelopes, n_env, signers, counts (as
        verify_frames_tally, the per-frame ones cut to n), seg_heads (wire.SegHead per segment), n_frames (total, not
        written) and, with want_index, off / flen."""
        from .wire import FrameHead, SegHead
        buf = np.ascontiguousarray(np.frombuffer(stream, np.uint8) if isinstance(stream, (bytes, bytearray))
                                   else stream, np.uint8).reshape(-1)
        seg_off = np.ascontiguousarray(seg_off, np.uint64).reshape(-1)
        seg_len = np.ascontiguousarray(seg_len, np.uint64).reshape(-1)
        s = len(seg_off)
        if len(seg_len) != s:
            raise ValueError("seg_off and seg_len must have the same length")
        if seg_peer is not None:
            seg_peer = np.ascontiguousarray(seg_peer, np.uint16).reshape(-1)
            if len(seg_peer) != s:
                raise ValueError("seg_peer must have one entry per segment")
        out = np.zeros((frame_cap + 63) // 64, dtype=np.uint64)
        heads = np.zeros(frame_cap, dtype=FrameHead)
        env_idx = np.zeros(frame_cap, dtype=np.uint32)
        envelopes = np.zeros((env_cap, 85), dtype=np.uint8)
        n_env = np.zeros(2, dtype=np.uint32)
        signers = np.zeros((env_cap, (self.n_keys + 63) // 64), dtype=np.uint64)
        counts = np.zeros(env_cap, dtype=np.uint32)
        seg_heads = np.zeros(s, dtype=SegHead)
        n_frames = np.zeros(2, dtype=np.uint32)
        off = np.zeros(frame_cap, dtype=np.uint64) if want_index else None
        flen = np.zeros(frame_cap, dtype=np.uint32) if want_index else None
        check(self._lib.pbft_verify_streams_tally(
            self._ctx, _ptr(buf), len(buf), _ptr(seg_off), _ptr(seg_len),
            _ptr(seg_peer) if seg_peer is not None else None, s,
            self.n_keys if n_replicas is None else n_replicas, frame_cap, env_cap, _ptr(out), _ptr(heads),
            _ptr(env_idx), _ptr(envelopes), n_env.ctypes.data, _ptr(signers), _ptr(counts), _ptr(seg_heads),
            n_frames.ctypes.data, _ptr(off) if want_index else None, _ptr(flen) if want_index else None))
        n = min(int(n_frames[0]), frame_cap)
        res = dict(n=n, bitmap=out[:(n + 63) // 64], heads=heads[:n], env_idx=env_idx[:n], envelopes=envelopes,
                   n_env=n_env, signers=signers, counts=counts, seg_heads=seg_heads, n_frames=n_frames)
        if want_index:
            res.update(off=off[:n], flen=flen[:n])
        return res

    def admit_reserve(self, log_window: int, n_keys: int, max_n: int) -> None:
        """pbft_admit_reserve: pre-size the admission workspace (required before capturing admit_device)."""
        check(self._lib.pbft_admit_reserve(self._ctx, log_window, n_keys, max_n))

    def admit_device(self, d_heads: int, d_records: int, n: int, view: int, h: int, log_window: int, n_keys: int,
                     residue_cap: int, d_class: int, d_counts: int, d_clean: int, d_res: int, d_n_res: int,
                     d_off: int = 0, d_len: int = 0, d_n_frames: int = 0, stream: int = 0) -> None:
        """pbft_admit_device: enqueue the replica's admission pass over n decoded frames (raw device pointers): class
        per frame, class counts, clean bitmap, residue list, and key index 0xFFFF into the record of every frame
        that is not clean -- see admit_reference."""
        check(self._lib.pbft_admit_device(self._ctx, d_heads or None, d_records or None, d_off or None, d_len or None,
                                          d_n_frames or None, n, view, h, log_window, n_keys, residue_cap,
                                          d_class or None, d_counts or None, d_clean or None, d_res or None,
                                          d_n_res or None, stream or None))

    OPT_INDEX_TILE = 19
    OPT_EGRESS_BLOCK, OPT_EGRESS_DIRECT = 20, 21
    OPT_PROPOSE_WIDTH = 22
    OPT_GROUP_SEED, OPT_GROUP_HASH_BITS = 16, 17
    OPT_SPLIT_BELOW, OPT_FINISH_WIDTH, OPT_KEY_TABLE_BUDGET_MB, OPT_FINISH_TREE, OPT_LAT_SPLIT = 1, 2, 3, 4, 5
    OPT_KERNEL_TIMING = 7
    OPT_FINISH_WAVES = 8
    OPT_COMB_PAIR = 10
    OPT_FAULT_INJECT = 11
    OPT_COMB_PRIO = 13
    OPT_COMB_BALANCE = 18

    def set_option(self, option: int, value: int) -> None:
        """pbft_verify_set_option: latency-mode threshold, finish width, key-table budget (include/pbft_verify.h)."""
        check(self._lib.pbft_verify_set_option(self._ctx, option, value))

    def positions(self) -> tuple[int, int]:
        """(PB, PA): comb positions (= steps) of the base-point plan and of the installed key set's plan."""
        pb, pa, nk = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        check(self._lib.pbft_verify_ctx_info(self._ctx, ctypes.byref(pb), ctypes.byref(pa), ctypes.byref(nk)))
        return pb.value, pa.value

    def last_kernel_ms(self) -> float:
        return float(self._lib.pbft_last_kernel_ms(self._ctx))

    # -- request digests (src/message.rs:209-212) and signing ---------------
    def _pack(self, items):
        lens = np.array([len(x) for x in items], dtype=np.uint32)
        offs = np.zeros(len(items), dtype=np.uint64)
        if len(items):
            offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
        data = np.frombuffer(b"".join(items) + bytes(16), dtype=np.uint8).copy()
        return data, offs, lens

    def blake2b512(self, items) -> np.ndarray:
        data, offs, lens = self._pack(items)
        out = np.zeros((len(items), 64), dtype=np.uint8)
        check(self._lib.pbft_digest_blake2b512(self._ctx, _ptr(data), _ptr(offs), _ptr(lens), len(items), _ptr(out)))
        return out

    def sha256(self, items) -> np.ndarray:
        data, offs, lens = self._pack(items)
        out = np.zeros((len(items), 32), dtype=np.uint8)
        check(self._lib.pbft_digest_sha256(self._ctx, _ptr(data), _ptr(offs), _ptr(lens), len(items), _ptr(out)))
        return out

    def sign(self, seeds: np.ndarray, seed_idx: np.ndarray, msg: np.ndarray, msg_len: int):
        """RFC 8032 signatures; returns (R, S, public_keys)."""
        seeds = np.ascontiguousarray(seeds, dtype=np.uint8).reshape(-1, 32)
        seed_idx = np.ascontiguousarray(seed_idx, dtype=np.uint16).reshape(-1)
        n = len(seed_idx)
        msg = np.ascontiguousarray(msg, dtype=np.uint8).reshape(n, -1) if n else np.zeros((0, 1), np.uint8)
        R = np.zeros((n, 32), dtype=np.uint8)
        S = np.zeros((n, 32), dtype=np.uint8)
        pub = np.zeros((len(seeds), 32), dtype=np.uint8)
        check(self._lib.pbft_sign_batch(self._ctx, _ptr(seeds), len(seeds), _ptr(seed_idx), _ptr(msg), msg_len,
                                        msg.shape[1], n, _ptr(R), _ptr(S), _ptr(pub)))
        return R, S, pub

    # -- egress: this replica's own votes, signed and framed on the GPU (include/pbft_wire.h) ------
    def set_signing_seed(self, seed, replica: int = 0) -> np.ndarray:
        """pbft_sign_set_seed: expand `seed` (32 bytes; None clears) once into the context's device-resident signing
        key; `replica` is the index the frames carry.  Returns the public key (zeros after a clear)."""
        pub = np.zeros(32, dtype=np.uint8)
        if seed is None:
            check(self._lib.pbft_sign_set_seed(self._ctx, None, 0, None))
            return pub
        sd = np.frombuffer(bytes(seed), dtype=np.uint8).copy()
        assert sd.size == 32
        check(self._lib.pbft_sign_set_seed(self._ctx, _ptr(sd), replica, _ptr(pub)))
        return pub

    def egress_reserve(self, max_n: int) -> None:
        """pbft_egress_reserve: pre-size the egress workspace (required before capturing sign_votes_frames_device
        into a graph)."""
        check(self._lib.pbft_egress_reserve(self._ctx, max_n))

    def sign_votes_frames(self, envelopes, env_stride: int = 85, with_sigs: bool = True):
        """pbft_sign_votes_frames: N envelopes (host, row i at i * env_stride) -> (stream, frame_off [N + 1], sigs
        [N][64] or None): the signed votes' UviBytes frames, what wire.encode_votes writes for them."""
        env = np.ascontiguousarray(envelopes, dtype=np.uint8).reshape(-1)
        n = 0 if env.size == 0 else (env.size - 85) // env_stride + 1
        need = ctypes.c_size_t()
        args = (self._ctx, _ptr(env) if n else None, env_stride, n)
        self._lib.pbft_sign_votes_frames(*args, None, 0, ctypes.byref(need), None, None)  # the size query
        out = np.zeros(max(need.value, 1), dtype=np.uint8)
        off = np.zeros(n + 1, dtype=np.uint64)
        sigs = np.zeros((n, 64), dtype=np.uint8) if with_sigs else None
        check(self._lib.pbft_sign_votes_frames(*args, _ptr(out), need.value, ctypes.byref(need), _ptr(off),
                                               _ptr(sigs) if with_sigs and n else None))
        return out[:need.value], off, sigs

    def sign_votes_frames_device(self, d_env: int, n: int, d_out: int, out_cap: int, d_frame_off: int,
                                 d_sigs: int = 0, env_stride: int = 85, stream: int = 0) -> None:
        """pbft_sign_votes_frames_device: enqueue only (raw device pointers): n envelopes at d_env -> the frames at
        d_out (any alignment, at most out_cap bytes, whole frames only), d_frame_off [n + 1] u64 and, if given,
        d_sigs [n][64]."""
        check(self._lib.pbft_sign_votes_frames_device(self._ctx, d_env or None, env_stride, n, d_out or None, out_cap,
                                                      d_frame_off or None, d_sigs or None, stream or None))

    # -- the primary's proposals: client requests hashed, signed and framed on the GPU (include/pbft_wire.h) ------
    def propose_reserve(self, max_n: int) -> None:
        """pbft_propose_reserve: pre-size the proposal workspace (required before capturing
        sign_preprepares_frames_device into a graph)."""
        check(self._lib.pbft_propose_reserve(self._ctx, max_n))

    def sign_preprepares_frames(self, view: int, first_seq: int, requests):
        """pbft_sign_preprepares_frames: `requests` (wire.pack_requests' tuple, host) -> (stream, frame_off [N + 1],
        digests [N][64], sigs [N][64], status [N]): the signed PrePrepares' UviBytes frames, what
        wire.encode_preprepares writes for them, under the identity of set_signing_seed."""
        data, ops_bytes, offs, lens, ts, cl = requests
        n = len(lens)
        need = ctypes.c_size_t()
        args = (self._ctx, _ptr(data), ops_bytes, _ptr(offs), _ptr(lens), _ptr(ts), _ptr(cl), view, first_seq, n)
        rc = self._lib.pbft_sign_preprepares_frames(*args, None, 0, ctypes.byref(need), None, None, None, None)
        if rc and not need.value:
            check(rc)
        out = np.zeros(max(need.value, 1), dtype=np.uint8)
        off = np.zeros(n + 1, dtype=np.uint64)
        dig, sigs = np.zeros((n, 64), dtype=np.uint8), np.zeros((n, 64), dtype=np.uint8)
        st = np.zeros(max(n, 1), dtype=np.uint8)
        check(self._lib.pbft_sign_preprepares_frames(*args, _ptr(out), need.value, ctypes.byref(need), _ptr(off),
                                                     _ptr(dig) if n else None, _ptr(sigs) if n else None, _ptr(st)))
        return out[:need.value], off, dig, sigs, st[:n]

    def sign_preprepares_frames_device(self, d_ops: int, ops_bytes: int, d_op_off: int, d_op_len: int, d_timestamp: int,
                                       d_clients: int, view: int, first_seq: int, n: int, d_out: int, out_cap: int,
                                       d_frame_off: int, d_digests: int, d_sigs: int, d_status: int,
                                       stream: int = 0) -> None:
        """pbft_sign_preprepares_frames_device: enqueue only (raw device pointers): n requests -> the canonical ones'
        frames at d_out (any alignment, at most out_cap bytes, whole frames only), d_frame_off [n + 1] u64, d_digests
        and d_sigs [n][64], d_status [n]."""
        check(self._lib.pbft_sign_preprepares_frames_device(
            self._ctx, d_ops or None, ops_bytes, d_op_off or None, d_op_len or None, d_timestamp or None,
            d_clients or None, view, first_seq, n, d_out or None, out_cap, d_frame_off or None, d_digests or None,
            d_sigs or None, d_status or None, stream or None))

    # -- client replies: results hashed with their clients, signed and written on the GPU (include/pbft_wire.h) ----
    def reply_reserve(self, max_n: int) -> None:
        """pbft_reply_reserve: pre-size the reply workspace (required before capturing sign_replies_device into a
        graph)."""
        check(self._lib.pbft_reply_reserve(self._ctx, max_n))

    def sign_replies(self, view: int, requests):
        """pbft_sign_replies: `requests` (wire.pack_results' tuple, host) -> (stream, reply_off [N + 1], digests [N][64],
        sigs [N][64], status [N]): the signed replies' texts back to back, what wire.encode_replies writes for them,
        under the identity of set_signing_seed."""
        data, nbytes, offs, lens, ts, cl = requests
        n = len(lens)
        need = ctypes.c_size_t()
        args = (self._ctx, _ptr(data), nbytes, _ptr(offs), _ptr(lens), _ptr(ts), _ptr(cl), view, n)
        check(self._lib.pbft_sign_replies(*args, None, 0, ctypes.byref(need), None, None, None, None))  # the size query
        out = np.zeros(max(need.value, 1), dtype=np.uint8)
        off = np.zeros(n + 1, dtype=np.uint64)
        dig, sigs = np.zeros((n, 64), dtype=np.uint8), np.zeros((n, 64), dtype=np.uint8)
        st = np.zeros(max(n, 1), dtype=np.uint8)
        check(self._lib.pbft_sign_replies(*args, _ptr(out), need.value, ctypes.byref(need), _ptr(off),
                                          _ptr(dig) if n else None, _ptr(sigs) if n else None, _ptr(st)))
        return out[:need.value], off, dig, sigs, st[:n]

    def sign_replies_device(self, d_results: int, results_bytes: int, d_res_off: int, d_res_len: int, d_timestamp: int,
                            d_clients: int, view: int, n: int, d_out: int, out_cap: int, d_reply_off: int,
                            d_digests: int, d_sigs: int, d_status: int, stream: int = 0) -> None:
        """pbft_sign_replies_device: enqueue only (raw device pointers): n executed requests -> the canonical replies'
        texts at d_out (any alignment, at most out_cap bytes, whole replies only), d_reply_off [n + 1] u64, d_digests
        and d_sigs [n][64], d_status [n]."""
        check(self._lib.pbft_sign_replies_device(
            self._ctx, d_results or None, results_bytes, d_res_off or None, d_res_len or None, d_timestamp or None,
            d_clients or None, view, n, d_out or None, out_cap, d_reply_off or None, d_digests or None, d_sigs or None,
            d_status or None, stream or None))

    # -- the client's side: signed replies matched, hashed, verified and tallied on the GPU (include/pbft_wire.h) ----
    def accept_reserve(self, max_n: int) -> None:
        """pbft_accept_reserve: build the PeerId table of the installed key set and size the blocking form's staging.
        Needed before the device forms, and again after set_keys / update_keys (with reserve(n) and group_reserve(n)
        before capturing accept_replies_device into a graph)."""
        check(self._lib.pbft_accept_reserve(self._ctx, max_n))

    def decode_replies_device(self, d_text: int, text_bytes: int, d_off: int, d_len: int, d_clients: int,
                              n_clients: int, n: int, d_records: int, d_heads: int, d_client_idx: int = 0,
                              stream: int = 0) -> None:
        """pbft_wire_decode_replies_device: enqueue only (raw device pointers; d_text 16-byte aligned): n reply texts ->
        d_records (n x 160 B) and d_heads (n x 32 B, wire.AcceptHead).  Texts that are not canonical are
        wire.ACCEPT_EDEFER."""
        check(self._lib.pbft_wire_decode_replies_device(self._ctx, d_text or None, text_bytes, d_off or None,
                                                        d_len or None, d_client_idx or None, d_clients or None,
                                                        n_clients, n, d_records or None, d_heads or None,
                                                        stream or None))

    def accept_replies_device(self, d_text: int, text_bytes: int, d_off: int, d_len: int, d_clients: int, n_clients: int,
                              n: int, need: int, d_records: int, d_heads: int, d_bitmap: int, env_cap: int,
                              d_env_idx: int, d_envelopes: int, d_n_env: int, d_signers: int, d_count: int, d_certs: int,
                              d_client_idx: int = 0, stream: int = 0) -> None:
        """pbft_accept_replies_device: decode, group, verify, tally and certify of n replies on one stream; d_certs is
        [env_cap] wire.AcceptCert."""
        check(self._lib.pbft_accept_replies_device(
            self._ctx, d_text or None, text_bytes, d_off or None, d_len or None, d_client_idx or None, d_clients or None,
            n_clients, n, need, d_records or None, d_heads or None, d_bitmap or None, env_cap, d_env_idx or None,
            d_envelopes or None, d_n_env or None, d_signers or None, d_count or None, d_certs or None, stream or None))

    def accept_replies(self, texts, clients, need: int, env_cap: int, client_idx=None, text_bytes: int | None = None,
                       want_env_idx: bool = True) -> dict:
        """pbft_accept_replies: the blocking, complete form.  texts: wire.pack_replies' tuple (buffer, off, len);
        clients: the client address fields (bytes or str each, or an (n_clients, 64) uint8 array); client_idx: None or
        one index per reply.  Returns a dict: bitmap (words), heads (wire.AcceptHead), env_idx or None, envelopes
        (env_cap, 85), n_env (2,), signers (env_cap, W), counts (env_cap,), certs (wire.AcceptCert): an envelope e with
        certs[e]["accepted"] is decided, and reply certs[e]["first"] holds its result."""
        from .wire import AcceptCert, AcceptHead, client_field
        buf, off, ln = texts
        buf = np.ascontiguousarray(buf, np.uint8).reshape(-1)
        off = np.ascontiguousarray(off, np.uint64).reshape(-1)
        ln = np.ascontiguousarray(ln, np.uint32).reshape(-1)
        n = len(off)
        if len(ln) != n:
            raise ValueError("off and len must have the same length")
        nbytes = int(ln.sum()) if text_bytes is None else text_bytes
        if isinstance(clients, np.ndarray):
            cl = np.ascontiguousarray(clients, np.uint8).reshape(-1, 64)
        else:
            cl = np.frombuffer(b"".join(client_field(c) for c in clients), np.uint8).reshape(-1, 64).copy()
        ci = None
        if client_idx is not None:
            ci = np.ascontiguousarray(client_idx, np.uint32).reshape(-1)
            if len(ci) != n:
                raise ValueError("client_idx must have one entry per reply")
        out = dict(bitmap=np.zeros((n + 63) // 64, np.uint64), heads=np.zeros(n, AcceptHead),
                   env_idx=np.zeros(n, np.uint32) if want_env_idx else None,
                   envelopes=np.zeros((env_cap, 85), np.uint8), n_env=np.zeros(2, np.uint32),
                   signers=np.zeros((env_cap, (self.n_keys + 63) // 64), np.uint64), counts=np.zeros(env_cap, np.uint32),
                   certs=np.zeros(env_cap, AcceptCert))
        check(self._lib.pbft_accept_replies(
            self._ctx, _ptr(buf), nbytes, _ptr(off), _ptr(ln), _ptr(ci) if ci is not None else None,
            _ptr(cl) if len(cl) else None, len(cl), n, need, env_cap, _ptr(out["bitmap"]), _ptr(out["heads"]),
            _ptr(out["env_idx"]) if want_env_idx else None, _ptr(out["envelopes"]), out["n_env"].ctypes.data,
            _ptr(out["signers"]), _ptr(out["counts"]), _ptr(out["certs"])))
        return out

    def close(self):
        if self._ctx:
            self._lib.pbft_verify_ctx_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
