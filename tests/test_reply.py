"""Client replies without a GPU: pbft_wire_encode_replies against the Python model of the reply text (pbft_amd/wire.py)
and against the canonical matcher (pbft_wire_decode_reply) in both directions; pbft_reply_digests against hashlib; the
PeerId text against pbft_key_from_peer_id_b58; pbft_replica_reply under a replier override (tests/reply_sim.py) on
replicas that ran a round to COMMITTED_LOCAL; and the text rule with the host encoder as a stand-alone program under
AddressSanitizer + UBSan (tests/native/reply_main.cpp)."""
import ctypes
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import reply_sim as R
from conftest import ROOT
from pbft_amd import wire
from replica_sim import Cluster, PhaseSim

VIEW = 1
PID = wire.peer_id_b58(bytes(range(32)))
# 0, 9, 10, every 10^k +- 1 and 2^64 - 1
WIDTHS = sorted({0, 9, 10, 2**64 - 1} | {10**k + d for k in range(1, 20) for d in (-1, 1)})


def encode(view, results, ts, replica, sigs=None, pid=PID):
    n = len(results)
    req = wire.pack_results(results, ts, [b"c"] * n)
    sg = np.random.default_rng(n).integers(0, 256, (n, 64), dtype=np.uint8) if sigs is None else sigs
    stream, off, st = wire.encode_replies(view, req, replica, pid, sg)
    assert int(off[0]) == 0 and int(off[-1]) == len(stream)
    return [stream[int(off[i]):int(off[i + 1])].tobytes() for i in range(n)], st, sg


def check_texts(view, results, ts, replica):
    texts, st, sg = encode(view, results, ts, replica)
    for i, t in enumerate(texts):
        assert t == wire.reply_text(view, ts[i], PID, results[i], replica, sg[i].tobytes()), (i, results[i][:8])
        can = wire.reply_canonical(results[i])
        assert int(st[i]) == (wire.REPLY_OK if can else wire.REPLY_GENERAL), i
        h = wire.decode_reply(t)
        assert (int(h["status"]) == wire.RH_OK) == can, i  # both directions
        if can:
            assert (int(h["view"]), int(h["timestamp"]), int(h["replica"])) == (view, ts[i], replica)
            assert t[int(h["result_off"]):int(h["result_off"]) + int(h["result_len"])] == results[i]
            assert bytes(h["peer_id"]) == PID and h["sig"].tobytes() == sg[i].tobytes()
        try:
            text = t.decode()
        except UnicodeDecodeError:
            continue
        j = json.loads(text)
        assert list(j) == ["view", "timestamp", "peer_id", "result", "replica", "signature"]
        assert (j["view"], j["timestamp"], j["replica"]) == (view, ts[i], replica)
        assert j["peer_id"] == PID.decode() and j["signature"] == sg[i].tobytes().hex()
        assert j["result"].encode() == results[i]
    return st


# ---- the encoder against the Python model ----
def test_symbols_exported():
    import pbft_amd
    lib = pbft_amd.load()
    for f in ("pbft_reply_digests", "pbft_wire_encode_replies", "pbft_wire_decode_reply", "pbft_reply_reserve",
              "pbft_sign_replies_device", "pbft_sign_replies"):
        assert hasattr(lib, f) and f in pbft_amd.EXPORTS
    for f in ("pbft_replica_reply", "pbft_replica_set_replier", "pbft_replica_set_last_timestamp",
              "pbft_replica_last_timestamp", "pbft_replica_get_reply_stats", "pbft_reply_envelope",
              "pbft_peer_id_b58_from_key"):
        assert hasattr(lib, f)


def test_result_lengths():
    results = [bytes(R.ALPHABET[np.arange(n) % len(R.ALPHABET)]) for n in R.RES_LENS]
    st = check_texts(3, results, list(range(1, len(results) + 1)), 2)
    assert list(st) == [0] * 10 + [1]  # 3,073 bytes: general


@pytest.mark.parametrize("special", R.SPECIALS)
def test_excluded_byte_classes_at_every_position(special):
    base = b"the result of the operation"
    results = []
    for at in (0, len(base) // 2, len(base) - len(special)):
        r = bytearray(base)
        r[at:at + len(special)] = special
        results.append(bytes(r))
    st = check_texts(1, results, [5, 6, 7], 0)
    assert list(st) == [1, 1, 1]


def test_other_controls_and_invalid_utf8():
    """\\b \\f \\n \\r \\t and \\u00xx as serde writes them; a result that is not valid UTF-8 is written as it stands
    (what pbft_wire_encode_preprepares does with such an operation)."""
    results = [bytes([c]) + b"x" for c in range(0x20)] + [b"\xff\xfe", b"a\x80"]
    st = check_texts(1, results, list(range(1, len(results) + 1)), 7)
    assert (st == 1).all()


def test_number_widths():
    for v in WIDTHS:
        check_texts(v, [b"awesome!"], [1], 2)
        check_texts(1, [b"awesome!"], [v], 2)
    for rep in (0, 9, 10, 65534):
        check_texts(10, [b"awesome!", b""], [10, 11], rep)


def test_mixed_batch():
    res, ts, cl = R.mixed_results(130)
    st = check_texts(VIEW, res, ts, 2)
    assert 30 < int((st == 0).sum()) < 130


# ---- encoder and decoder ----
def test_near_misses_are_none():
    texts, st, sg = encode(12, [b"awesome!"], [34], 5)
    good = texts[0]
    assert int(wire.decode_reply(good)["status"]) == wire.RH_OK
    sig_hex = sg[0].tobytes().hex().encode()
    letter = next(i for i, c in enumerate(sig_hex) if c in b"abcdef")
    upper = good.replace(sig_hex, sig_hex[:letter] + sig_hex[letter:letter + 1].upper() + sig_hex[letter + 1:])
    misses = {
        "a space": good.replace(b'"view":', b'"view": '),
        "another field order": good.replace(b'"view":12,"timestamp":34', b'"timestamp":34,"view":12'),
        "an escape": good.replace(b"awesome!", b"awesome\\u0021"),
        "a 51-character peer id": good.replace(PID, PID[:51]),
        "a 53-character peer id": good.replace(PID, PID + b"1"),
        "not base58": good.replace(PID, PID[:10] + b"0" + PID[11:]),
        "an uppercase hex digit": upper,
        "a trailing byte": good + b"\n",
        "a missing byte": good[:-1],
        "a leading zero": good.replace(b'"view":12', b'"view":012'),
        "a 21-digit number": good.replace(b'"view":12', b'"view":184467440737095516150'),
        "2^64": good.replace(b'"view":12', b'"view":18446744073709551616'),
        "replica 65536": good.replace(b'"replica":5', b'"replica":65536'),
        "a quote in the result": good.replace(b"awesome!", b'awe"some'),
        "empty": b"",
    }
    assert upper != good
    for name, t in misses.items():
        h = wire.decode_reply(t)
        assert int(h["status"]) == wire.RH_NONE and not h["sig"].any(), name
    long_ok, _, _ = encode(1, [b"x" * 3072, b"x" * 3073], [1, 2], 0)
    assert int(wire.decode_reply(long_ok[0])["status"]) == wire.RH_OK
    assert int(wire.decode_reply(long_ok[1])["status"]) == wire.RH_NONE  # (canonical but for its length)
    lib = wire.load()
    assert lib.pbft_wire_decode_reply(None, 5, np.zeros(1, wire.ReplyHead).ctypes.data) == R.EINVAL
    assert lib.pbft_wire_decode_reply(b"x", 1, None) == R.EINVAL


def test_length_query_and_short_cap():
    lib = wire.load()
    res, ts, cl = R.mixed_results(24, salt=3)
    req = wire.pack_results(res, ts, cl)
    data, _, off, ln, t, _ = req
    sig = np.zeros((24, 64), np.uint8)
    stream, roff, st = wire.encode_replies(3, req, 1, PID, sig)
    assert 0 < int((st == 0).sum()) < 24
    need = ctypes.c_size_t()
    args = (24, 3, t.ctypes.data, data.ctypes.data, off.ctypes.data, ln.ctypes.data, 1)
    r2, s2 = np.zeros(25, np.uint64), np.zeros(24, np.uint8)
    assert lib.pbft_wire_encode_replies(*args, None, None, None, 0, ctypes.byref(need), r2.ctypes.data,
                                        s2.ctypes.data) == 0
    assert need.value == len(stream) and (r2 == roff).all() and (s2 == st).all()
    pid = np.frombuffer(PID, np.uint8).copy()
    for cap in (len(stream) - 1, int(roff[7]) + 5, 1):  # PBFT_EINVAL, everything still reported, nothing behind cap
        out = np.full(len(stream) + 64, 0xA5, np.uint8)
        need.value = 0
        r2[:], s2[:] = 0, 9
        assert lib.pbft_wire_encode_replies(*args, pid.ctypes.data, sig.ctypes.data, out.ctypes.data, cap,
                                            ctypes.byref(need), r2.ctypes.data, s2.ctypes.data) == R.EINVAL
        assert need.value == len(stream) and (out[cap:] == 0xA5).all() and (r2 == roff).all() and (s2 == st).all()
    out = np.zeros(len(stream), np.uint8)
    assert lib.pbft_wire_encode_replies(*args, None, None, out.ctypes.data, len(stream), ctypes.byref(need), None,
                                        None) == R.EINVAL  # a real encode needs the peer id and the signatures
    assert lib.pbft_wire_encode_replies(*(args[:6] + (65536,)), None, None, None, 0, ctypes.byref(need), None,
                                        None) == R.EINVAL
    assert lib.pbft_wire_encode_replies(0, 1, None, None, None, None, 0, None, None, None, 0, ctypes.byref(need),
                                        r2.ctypes.data, None) == 0
    assert need.value == 0 and int(r2[0]) == 0


# ---- digests and the peer-id text ----
def test_reply_digests_against_hashlib():
    res, ts, cl = R.mixed_results(44)
    assert any(b"\0" in c for c in cl) and any(len(c) == 64 for c in cl) and any(len(c) == 0 for c in cl)
    req = wire.pack_results(res, ts, cl)
    got = wire.reply_digests(req)
    for i in range(44):
        c = cl[i].split(b"\0")[0]
        assert got[i].tobytes() == hashlib.blake2b(c + bytes(64 - len(c)) + res[i], digest_size=64).digest(), i
    # the client is bound: the same result under another client has another digest
    a = wire.reply_digests(wire.pack_results([b"r"], [1], [b"127.0.0.1:1"]))
    b = wire.reply_digests(wire.pack_results([b"r"], [1], [b"127.0.0.1:2"]))
    assert a.tobytes() != b.tobytes()
    data, nbytes, off, ln, _, c = req
    out = np.zeros((44, 64), np.uint8)
    assert wire.load().pbft_reply_digests(44, c.ctypes.data, data.ctypes.data, nbytes - 1, off.ctypes.data,
                                          ln.ctypes.data, out.ctypes.data) == R.EINVAL  # a result outside


def test_peer_id_text_inverts_on_the_extremes_and_random_keys():
    L = R.bind(wire.load())
    rng = np.random.default_rng(58)
    keys = [bytes(32), b"\xff" * 32] + [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(200)]
    for A in keys:
        out = ctypes.create_string_buffer(52)
        assert L.pbft_peer_id_b58_from_key(A, out) == 0
        text = out.raw
        assert len(text) == 52 and text == wire.peer_id_b58(A) and text.startswith(b"12D3KooW")
        back = ctypes.create_string_buffer(32)
        assert L.pbft_key_from_peer_id_b58(text, 52, back) == 0 and back.raw == A
    assert L.pbft_peer_id_b58_from_key(None, ctypes.create_string_buffer(52)) == R.EINVAL


def test_reply_envelope_is_kind_3():
    L = R.bind(wire.load())
    d = bytes(range(64))
    b = ctypes.create_string_buffer(85)
    L.pbft_reply_envelope(b, 2**64 - 2, 77, d)
    assert b.raw == b"PBFT\x03" + (2**64 - 2).to_bytes(8, "little") + (77).to_bytes(8, "little") + d


# ---- the replica ----
class Net(Cluster):
    """A 4-replica cluster whose seqs 1 .. n_seq are committed-local everywhere; replica `who` replies through the
    oracle override."""

    def __init__(self, n_seq=6, who=2, replier=True):
        super().__init__(4)
        R.bind(self.L)
        sim = PhaseSim(self)
        sim.start(VIEW, range(1, n_seq + 1))
        sim.run()
        assert all(sim.committed(i, VIEW, range(1, n_seq + 1)) for i in range(4))
        self.who = who
        self.replier = R.OracleReplier(self.L, self.o, self.seeds[who])
        if replier:
            self.replier.install(self.L, self.reps[who])

    def want(self, results, ts, cl):
        return R.reference(self.L, self.o, self.seeds[self.who], self.who, VIEW, results, ts, cl)


def test_replica_exactly_once_inside_a_batch_and_across_calls():
    c = Net()
    try:
        rep = c.reps[c.who]
        res = [b"r1", b"r2", b'a "general" one', b"r4", b"r5", b"r6"]
        ts = [5, 3, 7, 7, 6, 9]  # 3 is stale against 5; the second 7 and 6 against 7
        cl = [b"127.0.0.1:8080"] * 6
        req = wire.pack_results(res, ts, cl)
        rc, out, n, roff, st, nr = R.reply(c.L, rep, [1, 2, 3, 4, 5, 6], req)
        made = [0, 2, 5]
        _, stream, off, _, _, wst = c.want([res[i] for i in made], [ts[i] for i in made], [cl[i] for i in made])
        assert (rc, n, nr) == (0, len(stream), 3) and out.tobytes() == stream.tobytes()
        assert list(st) == [wire.REPLY_OK, wire.REPLY_STALE, wire.REPLY_GENERAL, wire.REPLY_STALE, wire.REPLY_STALE,
                            wire.REPLY_OK]
        assert [int(x) for x in roff] == [0, int(off[1]), int(off[1]), int(off[2]), int(off[2]), int(off[2]), len(stream)]
        assert R.last_timestamp(c.L, rep) == 9 and c.replier.calls == 1
        # across calls: everything up to 9 is stale now
        rc, out, n, roff, st, nr = R.reply(c.L, rep, [1, 2], wire.pack_results([b"a", b"b"], [9, 10], cl[:2]))
        assert (rc, nr) == (0, 1) and list(st) == [wire.REPLY_STALE, wire.REPLY_OK]
        assert out.tobytes() == c.want([b"b"], [10], cl[:1])[1].tobytes() and R.last_timestamp(c.L, rep) == 10
        s = R.reply_stats(c.L, rep)
        assert (s["replied"], s["calls"], s["stale"], s["not_committed"]) == (4, 2, 4, 0) and s["reply_ns"] > 0
        # a restart: the counter is the caller's to restore
        assert c.L.pbft_replica_set_last_timestamp(rep, 2) == 0
        assert R.reply(c.L, rep, [1], wire.pack_results([b"a"], [3], cl[:1]))[5] == 1
    finally:
        c.close()


def test_replica_uncommitted_and_garbage_collected_seqs():
    c = Net()
    try:
        rep = c.reps[c.who]
        cl = [b"10.0.0.7:1"] * 3
        req = wire.pack_results([b"x", b"y", b"z"], [1, 2, 3], cl)
        rc, out, n, roff, st, nr = R.reply(c.L, rep, [1, 7, 2], req)  # 7 was never proposed
        assert (rc, nr) == (0, 2) and list(st) == [wire.REPLY_OK, wire.REPLY_NOT_COMMITTED, wire.REPLY_OK]
        assert out.tobytes() == c.want([b"x", b"z"], [1, 3], cl[:2])[1].tobytes()
        assert R.last_timestamp(c.L, rep) == 3  # (the uncommitted entry's timestamp does not count)
        assert R.reply_stats(c.L, rep)["not_committed"] == 1
        # after the checkpoint the windows are gone; a seq this replica committed still counts, 7 .. still do not
        assert c.L.pbft_replica_stable_checkpoint(rep, 8) == 0
        assert c.L.pbft_replica_committed_local(rep, VIEW, 4) == 1 and c.L.pbft_replica_committed_local(rep, VIEW, 7) == 0
        rc, out, n, roff, st, nr = R.reply(c.L, rep, [4, 7, 8], wire.pack_results([b"x", b"y", b"z"], [4, 5, 6], cl))
        assert (rc, nr) == (0, 1) and list(st) == [wire.REPLY_OK, wire.REPLY_NOT_COMMITTED, wire.REPLY_NOT_COMMITTED]
    finally:
        c.close()


def test_replica_size_query_and_short_cap_change_nothing():
    c = Net()
    try:
        rep = c.reps[c.who]
        cl = [b"c"] * 3
        req = wire.pack_results([b"x", b"yy", b"zzz"], [4, 2, 6], cl)
        stream = c.want([b"x", b"zzz"], [4, 6], cl[:2])[1]
        data, nbytes, off, ln, ts, clf = req
        sq = np.array([1, 2, 3], np.uint64)
        need, nr = ctypes.c_size_t(), ctypes.c_uint64()
        roff, st = np.zeros(4, np.uint64), np.zeros(3, np.uint8)
        args = (rep, 3, sq.ctypes.data, ts.ctypes.data, clf.ctypes.data, data.ctypes.data, nbytes, off.ctypes.data,
                ln.ctypes.data, 0)
        assert c.L.pbft_replica_reply(*args, None, 0, ctypes.byref(need), roff.ctypes.data, st.ctypes.data,
                                      ctypes.byref(nr)) == 0
        assert (need.value, nr.value, list(st)) == (len(stream), 2, [0, wire.REPLY_STALE, 0]) and int(roff[3]) == len(stream)
        rc, out, n, roff2, st2, nr2 = R.reply(c.L, rep, sq, req, cap=len(stream) - 1)
        assert (rc, n, nr2) == (R.EINVAL, len(stream), 2) and list(st2) == list(st) and (roff2 == roff).all()
        assert R.last_timestamp(c.L, rep) == 0 and c.replier.calls == 0
        assert R.reply_stats(c.L, rep) == dict(replied=0, calls=0, stale=0, not_committed=0, reply_ns=0)
        rc, out, n, _, _, nr2 = R.reply(c.L, rep, sq, req, cap=len(stream))
        assert (rc, n, nr2) == (0, len(stream), 2) and out.tobytes() == stream.tobytes()
        # a result outside results_bytes, an unknown flag
        assert R.reply(c.L, rep, sq, (data, nbytes - 1, off, ln, ts, clf), cap=1 << 12)[0] == R.EINVAL
        assert R.reply(c.L, rep, sq, req, cap=1 << 12, flags=1)[0] == R.EINVAL
    finally:
        c.close()


def test_replica_without_a_replier_or_a_seed_is_an_error():
    c = Net(replier=False)
    try:
        rep = c.reps[c.who]
        req = wire.pack_results([b"x"], [4], [b"c"])
        assert R.reply(c.L, rep, [1], req)[0] == R.EINVAL  # (the size query inside needs no signer; the call does)
        assert R.last_timestamp(c.L, rep) == 0
        c.replier.install(c.L, rep)
        assert R.reply(c.L, rep, [1], req)[5] == 1
        assert c.L.pbft_replica_set_replier(rep, R.REPLIER_FN(), None) == 0  # removed again
        assert R.reply(c.L, rep, [1], wire.pack_results([b"x"], [5], [b"c"]))[0] == R.EINVAL
    finally:
        c.close()


# ---- the stand-alone sanitizer run ----
NATIVE = os.path.join(ROOT, "tests", "native")
BIN = os.path.join(NATIVE, "reply_main")
CSRC = os.path.join(ROOT, "pbft_amd", "csrc")
SRCS = [os.path.join(NATIVE, "reply_main.cpp"), os.path.join(CSRC, "host", "wire.cpp"),
        os.path.join(CSRC, "host", "replica.cpp")]
DEPS = SRCS + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + \
       [os.path.join(ROOT, "include", f) for f in os.listdir(os.path.join(ROOT, "include"))]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]


def test_text_rule_encoder_and_replica_clean_under_asan_ubsan():
    if not (os.path.exists(BIN) and all(os.path.getmtime(d) <= os.path.getmtime(BIN) for d in DEPS)):
        if not os.path.exists(HIPCC):
            pytest.skip("hipcc not present")
        subprocess.run([HIPCC, "--offload-host-only", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-pthread"] +
                       SAN + ["-o", BIN] + SRCS, check=True, timeout=900)
    env = dict(os.environ)
    sym = "/opt/rocm/lib/llvm/bin/llvm-symbolizer"
    if os.path.exists(sym):
        env["ASAN_SYMBOLIZER_PATH"] = sym
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0:halt_on_error=1"
    p = subprocess.run([BIN, "300"], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    m = re.search(r"reply host run ok: (\d+) replies, (\d+) canonical, (\d+) through the replica", p.stdout)
    assert m and int(m.group(1)) > 800 and 100 < int(m.group(2)) < int(m.group(1)) and int(m.group(3)) > 100
