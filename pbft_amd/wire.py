"""ctypes binding of the wire codec (include/pbft_wire.h, pbft_amd/csrc/host/wire.cpp).

Plumbing for tests and tools: UviBytes framing + serde_json Message encoding of
the reference (src/protocol_config.rs:41-129, src/message.rs:7-31) with the
signed-envelope fields, and the stream -> struct-of-arrays vote decoder that
feeds the GPU verifier.  The codec itself is the C++ library code.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np

from ._lib import PbftError, check, load

PREPREPARE, PREPARE, COMMIT, CLIENT_REQUEST = 0, 1, 2, 3
RECORD_BYTES = 160
ENVELOPE = 85
STATUS = {0: "ok", 1: "json", 2: "digest", 3: "unsigned", 4: "kind", 5: "signer", 6: "defer"}
EDEFER = 6  # PBFT_WIRE_EDEFER: not the canonical vote form (device decode only; verify_frames settles it)
FRAME_MIN, FRAME_MAX = 336, 379  # byte lengths of a canonical signed vote
# pbft_frame_head (include/pbft_wire.h): one per frame of decode_frames_device / verify_frames
FrameHead = np.dtype([("view", "<u8"), ("seq", "<u8"), ("key_idx", "<u2"), ("kind", "u1"), ("status", "u1"),
                      ("frame_len", "<u4")])
assert FrameHead.itemsize == 24
# pbft_seg_head (include/pbft_wire.h): one per segment of index_streams_device / verify_streams_tally
SegHead = np.dtype([("consumed", "<u8"), ("first", "<u4"), ("n_frames", "<u4"), ("status", "<u4"), ("pad", "<u4")])
assert SegHead.itemsize == 24
# pbft_admit_residue (include/pbft_wire.h): one frame the replica's host code has to see, 16 bytes
AdmitResidue = np.dtype([("off", "<u8"), ("frame", "<u4"), ("len", "<u4")])
assert AdmitResidue.itemsize == 16
SEG_OK, SEG_EFRAMING, SEG_EOUTSIDE = 0, 1, 2  # PBFT_SEG_*
# pbft_pp_head (include/pbft_wire.h): one per residue entry of decode_preprepares_device / verify_streams_admit_pp
PpHead = np.dtype([("view", "<u8"), ("seq", "<u8"), ("timestamp", "<u8"), ("op_off", "<u4"), ("op_len", "<u4"),
                   ("replica", "<u2"), ("status", "u1"), ("pad", "u1", 5), ("claimed", "u1", 64),
                   ("computed", "u1", 64), ("sig", "u1", 64)])
assert PpHead.itemsize == 232
PP_NONE, PP_OK = 0, 1  # PBFT_PP_*
PP_OP_MAX = 3072
PP_FRAME_MIN, PP_FRAME_MAX = 394, 517 + PP_OP_MAX  # byte lengths of a canonical signed PrePrepare


class _Msg(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_uint32), ("view", ctypes.c_uint64), ("seq", ctypes.c_uint64),
                ("digest", ctypes.c_uint8 * 64), ("digest_ok", ctypes.c_uint32), ("has_sig", ctypes.c_uint32),
                ("replica", ctypes.c_uint32), ("sig", ctypes.c_uint8 * 64), ("operation", ctypes.c_void_p),
                ("operation_len", ctypes.c_uint32), ("timestamp", ctypes.c_uint64), ("client", ctypes.c_char * 64)]


@dataclass
class WireMsg:
    kind: int
    view: int = 0
    seq: int = 0
    digest: bytes = bytes(64)
    replica: int | None = None      # signed-envelope extension
    sig: bytes | None = None        # R || S
    operation: bytes = b""          # ClientRequest (standalone or inside PrePrepare)
    timestamp: int = 0
    client: str = ""
    digest_ok: bool = True
    _keep: list = field(default_factory=list, repr=False)

    def _to_c(self) -> _Msg:
        m = _Msg()
        m.kind, m.view, m.seq = self.kind, self.view, self.seq
        ctypes.memmove(m.digest, bytes(self.digest), 64)
        m.digest_ok = 1
        if self.sig is not None:
            m.has_sig, m.replica = 1, int(self.replica or 0)
            ctypes.memmove(m.sig, bytes(self.sig), 64)
        buf = ctypes.create_string_buffer(bytes(self.operation), max(1, len(self.operation)))
        self._keep = [buf]
        m.operation = ctypes.cast(buf, ctypes.c_void_p)
        m.operation_len = len(self.operation)
        m.timestamp = self.timestamp
        m.client = self.client.encode()
        return m


def uvi_encode(v: int) -> bytes:
    out = (ctypes.c_uint8 * 10)()
    n = load().pbft_uvi_encode(v, out)
    return bytes(out[:n])


def uvi_decode(buf: bytes):
    """(value, header_bytes) | None if more bytes are needed; raises on invalid."""
    v, h = ctypes.c_uint64(), ctypes.c_size_t()
    b = (ctypes.c_uint8 * max(1, len(buf))).from_buffer_copy(buf or b"\0")
    rc = load().pbft_uvi_decode(b, len(buf), ctypes.byref(v), ctypes.byref(h))
    if rc == 1:
        return None
    check(rc)
    return v.value, h.value


def encode_json(m: WireMsg) -> bytes:
    lib, cm = load(), m._to_c()
    n = ctypes.c_size_t()
    lib.pbft_wire_encode_json(ctypes.byref(cm), None, 0, ctypes.byref(n))
    out = ctypes.create_string_buffer(n.value)
    check(lib.pbft_wire_encode_json(ctypes.byref(cm), out, n.value, ctypes.byref(n)))
    return out.raw[: n.value]


def encode_frame(m: WireMsg) -> bytes:
    lib, cm = load(), m._to_c()
    n = ctypes.c_size_t()
    lib.pbft_wire_encode_frame(ctypes.byref(cm), None, 0, ctypes.byref(n))
    out = ctypes.create_string_buffer(n.value)
    check(lib.pbft_wire_encode_frame(ctypes.byref(cm), out, n.value, ctypes.byref(n)))
    return out.raw[: n.value]


def decode_json(js: bytes) -> WireMsg:
    lib = load()
    cm = _Msg()
    arena = ctypes.create_string_buffer(len(js) + 16)
    src = ctypes.create_string_buffer(bytes(js), max(1, len(js)))
    rc = lib.pbft_wire_decode_json(src, len(js), ctypes.byref(cm), arena, len(js) + 16)
    if rc:
        raise PbftError(rc, "not a Message of the reference schema")
    op = ctypes.string_at(cm.operation, cm.operation_len) if cm.operation_len else b""
    return WireMsg(kind=cm.kind, view=cm.view, seq=cm.seq, digest=bytes(cm.digest),
                   replica=cm.replica if cm.has_sig else None, sig=bytes(cm.sig) if cm.has_sig else None,
                   operation=op, timestamp=cm.timestamp, client=cm.client.decode(), digest_ok=bool(cm.digest_ok))


def decode_preprepare(body: bytes) -> np.ndarray:
    """pbft_wire_decode_preprepare: the canonical-PrePrepare rule and the operation's digest for one frame body, on the
    host.  Returns one PpHead record (status PP_OK, or all zero: the general parser decides)."""
    out = np.zeros(1, PpHead)
    src = ctypes.create_string_buffer(bytes(body), max(1, len(body)))
    check(load().pbft_wire_decode_preprepare(src, len(body), out.ctypes.data))
    return out[0]


@dataclass
class Votes:
    status: np.ndarray   # per decoded frame (STATUS)
    R: np.ndarray
    S: np.ndarray
    key_idx: np.ndarray
    msg: np.ndarray      # (rows, 85) envelopes
    kind: np.ndarray
    view: np.ndarray
    seq: np.ndarray
    consumed: int        # bytes of whole frames


def decode_votes(stream: bytes, n_replicas: int, max_frames: int | None = None) -> Votes:
    lib = load()
    cap = max(1, len(stream) // 8 + 1) if max_frames is None else max_frames
    st = np.zeros(cap, np.uint8)
    R, S = np.zeros((cap, 32), np.uint8), np.zeros((cap, 32), np.uint8)
    K, M = np.zeros(cap, np.uint16), np.zeros((cap, ENVELOPE), np.uint8)
    kd, vw, sq = np.zeros(cap, np.uint8), np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
    nf, nr, used = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    buf = np.frombuffer(bytes(stream) or b"\0", np.uint8)
    check(lib.pbft_wire_decode_votes(buf.ctypes.data, len(stream), n_replicas, cap, cap, st.ctypes.data,
                                     R.ctypes.data, S.ctypes.data, K.ctypes.data, M.ctypes.data, kd.ctypes.data,
                                     vw.ctypes.data, sq.ctypes.data, ctypes.byref(nf), ctypes.byref(nr),
                                     ctypes.byref(used)))
    f, r = nf.value, nr.value
    return Votes(st[:f], R[:r], S[:r], K[:r], M[:r], kd[:r], vw[:r], sq[:r], used.value)


def frame_index(stream, max_frames: int | None = None):
    """pbft_wire_frame_index: the varint scan of a stream of UviBytes frames; returns (off uint64[n], flen uint32[n],
    consumed): frame f's body is stream[off[f] : off[f] + flen[f]], consumed the bytes of whole frames.  Raises on a
    framing error."""
    buf = np.ascontiguousarray(np.frombuffer(stream, np.uint8) if isinstance(stream, (bytes, bytearray))
                               else stream, np.uint8).reshape(-1)
    cap = len(buf) if max_frames is None else max_frames  # (a frame is at least its one varint byte)
    off, flen = np.zeros(max(1, cap), np.uint64), np.zeros(max(1, cap), np.uint32)
    nf, used = ctypes.c_uint64(), ctypes.c_uint64()
    check(load().pbft_wire_frame_index(buf.ctypes.data if len(buf) else None, len(buf), cap, off.ctypes.data,
                                       flen.ctypes.data, ctypes.byref(nf), ctypes.byref(used)))
    return off[: nf.value].copy(), flen[: nf.value].copy(), used.value


def records_pack(R, S, key_idx, msg, msg_stride: int = ENVELOPE) -> np.ndarray:
    n = len(R)
    out = np.zeros((n, RECORD_BYTES), np.uint8)
    R, S = np.ascontiguousarray(R, np.uint8), np.ascontiguousarray(S, np.uint8)
    K, M = np.ascontiguousarray(key_idx, np.uint16), np.ascontiguousarray(msg, np.uint8)
    check(load().pbft_records_pack(R.ctypes.data, S.ctypes.data, K.ctypes.data, M.ctypes.data, msg_stride, n,
                                   out.ctypes.data))
    return out


def encode_votes(kind, view, seq, digests, replica, sigs) -> np.ndarray:
    """N signed votes as one stream of UviBytes/JSON frames (include/pbft_wire.h pbft_wire_encode_votes): what one
    connection carries (uint8 array)."""
    lib = load()
    k = np.ascontiguousarray(kind, np.uint8)
    v, q = np.ascontiguousarray(view, np.uint64), np.ascontiguousarray(seq, np.uint64)
    d, s = np.ascontiguousarray(digests, np.uint8), np.ascontiguousarray(sigs, np.uint8)
    r = np.ascontiguousarray(replica, np.uint32)
    n = ctypes.c_size_t()
    args = (len(k), k.ctypes.data, v.ctypes.data, q.ctypes.data, d.ctypes.data, r.ctypes.data, s.ctypes.data)
    lib.pbft_wire_encode_votes(*args, None, 0, ctypes.byref(n))
    out = np.zeros(max(1, n.value), np.uint8)
    check(lib.pbft_wire_encode_votes(*args, out.ctypes.data, n.value, ctypes.byref(n)))
    return out[: n.value]


PROPOSE_OK, PROPOSE_GENERAL = 0, 1  # PBFT_PROPOSE_*


def pack_requests(ops, timestamps, clients):
    """Client requests as the arrays the proposal entry points take: (data uint8 -- the operations back to back, padded
    to a 16-byte multiple --, ops_bytes, op_off uint64[n], op_len uint32[n], timestamp uint64[n], clients uint8[n][64]:
    each client's bytes, NUL-padded; 64 bytes leave no NUL)."""
    ops = [bytes(o) for o in ops]
    n = len(ops)
    lens = np.array([len(o) for o in ops], np.uint32)
    offs = np.zeros(n, np.uint64)
    if n:
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    raw = b"".join(ops)
    data = np.frombuffer(raw + bytes((-len(raw)) % 16 or (0 if raw else 16)), np.uint8).copy()
    cl = np.zeros((n, 64), np.uint8)
    for i, c in enumerate(clients):
        c = c.encode() if isinstance(c, str) else bytes(c)
        assert len(c) <= 64
        cl[i, :len(c)] = np.frombuffer(c, np.uint8)
    return data, len(raw), offs, lens, np.ascontiguousarray(timestamps, np.uint64).reshape(n), cl


def encode_preprepares(view: int, first_seq: int, requests, replica: int, digests, sigs):
    """pbft_wire_encode_preprepares: the signed PrePrepares of `requests` (pack_requests' tuple) with sequence numbers
    first_seq, first_seq + 1, ... as one stream of UviBytes/JSON frames.  Returns (stream uint8, frame_off uint64[n + 1],
    status uint8[n]: PROPOSE_OK for the canonical form, PROPOSE_GENERAL for any other request)."""
    lib = load()
    data, _, offs, lens, ts, cl = requests
    n = len(lens)
    d = np.ascontiguousarray(digests, np.uint8).reshape(n, 64)
    s = np.ascontiguousarray(sigs, np.uint8).reshape(n, 64)
    need = ctypes.c_size_t()
    off, st = np.zeros(n + 1, np.uint64), np.zeros(max(n, 1), np.uint8)
    args = (n, view, first_seq, data.ctypes.data, offs.ctypes.data, lens.ctypes.data, ts.ctypes.data, cl.ctypes.data,
            replica)
    check(lib.pbft_wire_encode_preprepares(*args, None, None, None, 0, ctypes.byref(need), None, None))
    out = np.zeros(max(1, need.value), np.uint8)
    check(lib.pbft_wire_encode_preprepares(*args, d.ctypes.data, s.ctypes.data, out.ctypes.data, need.value,
                                           ctypes.byref(need), off.ctypes.data, st.ctypes.data))
    return out[: need.value], off, st[:n]


# ---- client replies (include/pbft_wire.h; text rule: pbft_amd/csrc/reply_core.h) ----
KIND_REPLY = 3  # PBFT_KIND_REPLY
REPLY_OK, REPLY_GENERAL, REPLY_STALE, REPLY_NOT_COMMITTED = 0, 1, 2, 3  # PBFT_REPLY_*
REPLY_RESULT_MAX = 3072
RH_NONE, RH_OK = 0, 1  # PBFT_RH_*
# pbft_reply_head (include/pbft_wire.h): what decode_reply answers
ReplyHead = np.dtype([("view", "<u8"), ("timestamp", "<u8"), ("result_off", "<u4"), ("result_len", "<u4"),
                      ("replica", "<u4"), ("status", "<u4"), ("peer_id", "S52"), ("sig", "u1", 64), ("pad", "u1", 4)])
assert ReplyHead.itemsize == 152
_B58 = b"123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"
_SERDE_SHORT = {0x22: b'\\"', 0x5C: b"\\\\", 0x08: b"\\b", 0x0C: b"\\f", 0x0A: b"\\n", 0x0D: b"\\r", 0x09: b"\\t"}


def serde_escape(s: bytes) -> bytes:
    """The body of a JSON string as serde_json writes it: `"` and `\\` escaped, control characters as \\b \\f \\n \\r
    \\t or \\u00xx, every other byte (0x7F and UTF-8 sequences included) as it is."""
    out = bytearray()
    for c in bytes(s):
        if c in _SERDE_SHORT:
            out += _SERDE_SHORT[c]
        elif c < 0x20:
            out += b"\\u00%02x" % c
        else:
            out.append(c)
    return bytes(out)


def peer_id_b58(pub: bytes) -> bytes:
    """The PeerId text of an Ed25519 key: base58btc of 00 24 08 01 12 20 | A (a Python model of
    pbft_peer_id_b58_from_key)."""
    raw = bytes([0x00, 0x24, 0x08, 0x01, 0x12, 0x20]) + bytes(pub)
    v, out = int.from_bytes(raw, "big"), bytearray()
    while v:
        v, r = divmod(v, 58)
        out.append(_B58[r])
    out += b"1" * (len(raw) - len(raw.lstrip(b"\0")))
    return bytes(out[::-1])


def reply_canonical(result: bytes) -> bool:
    return len(result) <= REPLY_RESULT_MAX and all(0x20 <= c <= 0x7E and c not in (0x22, 0x5C) for c in bytes(result))


def reply_text(view: int, timestamp: int, peer_id: bytes, result: bytes, replica: int, sig: bytes) -> bytes:
    """A Python model of one signed reply's text: the reference's ClientReply serialization (src/message.rs:54-103) in
    its field order, then "replica" and "signature"."""
    return b'{"view":%d,"timestamp":%d,"peer_id":"%s","result":"%s","replica":%d,"signature":"%s"}' % (
        view, timestamp, bytes(peer_id), serde_escape(result), replica, bytes(sig).hex().encode())


def client_field(client) -> bytes:
    """C of the reply digest: the client's 64-byte field with everything from its first NUL on replaced by zeros."""
    c = client.encode() if isinstance(client, str) else bytes(client)
    c = c[:64].split(b"\0")[0]
    return c + bytes(64 - len(c))


# Executed requests as the arrays the reply entry points take: pack_requests' tuple, the results in the operations' place.
pack_results = pack_requests


def reply_digests(requests) -> np.ndarray:
    """pbft_reply_digests: D = Blake2b-512(C | result) per reply, uint8[n][64]."""
    data, nbytes, offs, lens, _, cl = requests
    n = len(lens)
    out = np.zeros((n, 64), np.uint8)
    check(load().pbft_reply_digests(n, cl.ctypes.data, data.ctypes.data, nbytes, offs.ctypes.data, lens.ctypes.data,
                                    out.ctypes.data))
    return out


def encode_replies(view: int, requests, replica: int, peer_id: bytes, sigs):
    """pbft_wire_encode_replies: the signed replies of `requests` (pack_results' tuple) back to back.  Returns (stream
    uint8, reply_off uint64[n + 1], status uint8[n]: REPLY_OK for the canonical form, REPLY_GENERAL for any other)."""
    lib = load()
    data, _, offs, lens, ts, _ = requests
    n = len(lens)
    s = np.ascontiguousarray(sigs, np.uint8).reshape(n, 64)
    pid = np.frombuffer(bytes(peer_id), np.uint8).copy()
    assert len(pid) == 52
    need = ctypes.c_size_t()
    off, st = np.zeros(n + 1, np.uint64), np.zeros(max(n, 1), np.uint8)
    args = (n, view, ts.ctypes.data, data.ctypes.data, offs.ctypes.data, lens.ctypes.data, replica)
    check(lib.pbft_wire_encode_replies(*args, None, None, None, 0, ctypes.byref(need), None, None))
    out = np.zeros(max(1, need.value), np.uint8)
    check(lib.pbft_wire_encode_replies(*args, pid.ctypes.data, s.ctypes.data, out.ctypes.data, need.value,
                                       ctypes.byref(need), off.ctypes.data, st.ctypes.data))
    return out[: need.value], off, st[:n]


def decode_reply(text: bytes) -> np.ndarray:
    """pbft_wire_decode_reply: the canonical-reply matcher for one text.  Returns one ReplyHead record (status RH_OK, or
    all zero: a general JSON parser decides)."""
    out = np.zeros(1, ReplyHead)
    src = ctypes.create_string_buffer(bytes(text), max(1, len(text)))
    check(load().pbft_wire_decode_reply(src, len(text), out.ctypes.data))
    return out[0]


# ---- the client's side: signed replies in, f + 1 results out (include/pbft_wire.h; rule: pbft_amd/csrc/accept_core.h) ----
ACCEPT_OK, ACCEPT_EDEFER, ACCEPT_ESIGNER, ACCEPT_ECLIENT, ACCEPT_EJSON = range(5)  # PBFT_ACCEPT_*
ACCEPT_ESCAPED = 0x100   # a flag beside ACCEPT_OK: the raw span [result_off, result_off + result_len) holds an escape
ACCEPT_NO_REPLY = 0xFFFFFFFF
RH_GENERAL = 2  # PBFT_RH_GENERAL: decode_reply_json's status for a text that is not canonical
# pbft_accept_head: one per reply of decode_replies_device / accept_replies
AcceptHead = np.dtype([("view", "<u8"), ("timestamp", "<u8"), ("result_off", "<u4"), ("result_len", "<u4"),
                       ("replica", "<u4"), ("status", "<u4")])
assert AcceptHead.itemsize == 32
# pbft_accept_cert: one per envelope of accept_replies_device / accept_replies
AcceptCert = np.dtype([("view", "<u8"), ("timestamp", "<u8"), ("first", "<u4"), ("count", "<u4"), ("client", "<u4"),
                       ("accepted", "<u4")])
assert AcceptCert.itemsize == 32


def pack_replies(texts):
    """Reply texts (bytes each) back to back -> (buffer uint8 padded to a multiple of 16, off uint64[n], len
    uint32[n]): the arrays the acceptance entry points take; the texts' bytes are sum(len)."""
    lens = np.array([len(t) for t in texts], np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens, dtype=np.uint64)[:-1]]).astype(np.uint64) if len(texts) else \
        np.zeros(0, np.uint64)
    raw = b"".join(bytes(t) for t in texts)
    buf = np.zeros((len(raw) + 15) // 16 * 16 + 16, np.uint8)
    buf[:len(raw)] = np.frombuffer(raw, np.uint8)
    return buf, offs, lens


def decode_reply_json(text: bytes):
    """pbft_wire_decode_reply_json: the serde-exact reader of one signed reply.  Returns (ReplyHead record, result bytes
    with their escapes decoded), or None for a text that is not a signed ClientReply.  status is RH_OK on a canonical
    text (the record is decode_reply's) and RH_GENERAL on any other, where result_off / result_len give the raw span
    between the result's quotes."""
    out = np.zeros(1, ReplyHead)
    src = ctypes.create_string_buffer(bytes(text), max(1, len(text)))
    arena = ctypes.create_string_buffer(max(1, len(text)))
    rc = load().pbft_wire_decode_reply_json(src, len(text), out.ctypes.data, arena, len(text))
    if rc < 0:
        return None
    return out[0], arena.raw[:rc]
