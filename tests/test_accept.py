"""The client's side without a GPU: pbft_wire_decode_reply_json against `json` on the acceptance corpus
(tests/accept_sim.py) and against pbft_wire_decode_reply on its canonical part, with the texts serde refuses; the Python
model pbft_amd.accept_reference on hand-checked cases and the conditions the corpus has to meet; and the parser with
accept_core.h's host build as a stand-alone program under AddressSanitizer + UBSan (tests/native/accept_main.cpp)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import accept_sim as A
from conftest import ROOT
from pbft_amd import accept_reference, wire


def test_symbols_exported():
    import pbft_amd
    lib = pbft_amd.load()
    for f in ("pbft_wire_decode_reply_json", "pbft_accept_reserve", "pbft_wire_decode_replies_device",
              "pbft_accept_replies_device", "pbft_accept_replies"):
        assert hasattr(lib, f) and f in pbft_amd.EXPORTS


# ---- the general reader ----
def check_against_json(t):
    """decode_reply_json(t) against json.loads(t); returns whether it parsed."""
    got = wire.decode_reply_json(t)
    can = wire.decode_reply(t)
    try:
        j = json.loads(t.decode("utf-8"))
        j["result"].encode("utf-8")
    except (ValueError, KeyError, TypeError, AttributeError):
        j = None
    if got is None:
        assert int(can["status"]) == wire.RH_NONE
        return False
    h, res = got
    assert j is not None, t[:60]
    assert (int(h["view"]), int(h["timestamp"]), int(h["replica"])) == (j["view"], j["timestamp"], j["replica"])
    assert bytes(h["peer_id"]) == j["peer_id"].encode() and h["sig"].tobytes().hex() == j["signature"]
    assert res == j["result"].encode("utf-8")
    raw = t[int(h["result_off"]):int(h["result_off"]) + int(h["result_len"])]
    assert json.loads(b'"' + raw + b'"') == j["result"]
    if int(can["status"]) == wire.RH_OK:  # the canonical part: the same record
        assert h.tobytes() == can.tobytes() and raw == res
    else:
        assert int(h["status"]) == wire.RH_GENERAL
    return True


def test_reader_against_json_on_the_corpus():
    c = A.corpus(85, with_outside=False)
    m = A.model(c, settle=True)
    parsed = [check_against_json(t) for t in c["texts"]]
    assert [bool(p) for p in parsed] == [int(s) & 0xFF != wire.ACCEPT_EJSON for s in m["heads"]["status"]]
    assert 10 < parsed.count(False) < 20 and sum(b"\\" in t for t, p in zip(c["texts"], parsed) if p) > 20


def test_reader_returns_what_the_encoder_was_given():
    res, ts, cl = A.R.mixed_results(130)
    res = [r for r in res if len(r) <= 3072 or wire.reply_canonical(r[:1])]
    n = len(res)
    sg = np.random.default_rng(5).integers(0, 256, (n, 64), dtype=np.uint8)
    pid = wire.peer_id_b58(bytes(range(32)))
    stream, off, st = wire.encode_replies(7, wire.pack_results(res, ts[:n], cl[:n]), 3, pid, sg)
    assert 0 < int((st == 1).sum()) < n
    for i in range(n):
        t = stream[int(off[i]):int(off[i + 1])].tobytes()
        try:
            res[i].decode("utf-8")
        except UnicodeDecodeError:
            assert wire.decode_reply_json(t) is None  # (serde could not have produced such a String)
            continue
        h, r = wire.decode_reply_json(t)
        assert r == res[i] and (int(h["view"]), int(h["timestamp"]), int(h["replica"])) == (7, ts[i], 3)
        assert bytes(h["peer_id"]) == pid and h["sig"].tobytes() == sg[i].tobytes()
        assert int(h["status"]) == (wire.RH_OK if st[i] == 0 else wire.RH_GENERAL)


GOOD = b'{"view":12,"timestamp":34,"peer_id":"%s","result":"awesome!","replica":5,"signature":"%s"}' % (
    wire.peer_id_b58(bytes(range(32))), bytes(range(64)).hex().encode())
PID = wire.peer_id_b58(bytes(range(32)))


def test_reader_rejects_what_serde_rejects():
    assert check_against_json(GOOD)
    sig = bytes(range(64)).hex().encode()
    bad = {
        "a duplicate field": GOOD.replace(b'"view":12,', b'"view":12,"view":12,'),
        "a duplicate result": GOOD.replace(b'"replica":5', b'"result":"x","replica":5'),
        "a 51-character peer id": GOOD.replace(PID, PID[:51]),
        "a 53-character peer id": GOOD.replace(PID, PID + b"1"),
        "a 127-character signature": GOOD.replace(sig, sig[:127]),
        "an uppercase hex digit": GOOD.replace(sig, sig.upper()),  # (as pbft_wire_decode_json: lowercase only)
        "replica 65536": GOOD.replace(b'"replica":5', b'"replica":65536'),
        "a 21-digit number": GOOD.replace(b'"view":12', b'"view":184467440737095516150'),
        "2^64": GOOD.replace(b'"timestamp":34', b'"timestamp":18446744073709551616'),
        "a trailing byte": GOOD + b"x",
        "a trailing object": GOOD + b"{}",
        "a lone surrogate escape": GOOD.replace(b"awesome!", b"awe\\ud800some"),
        "a lone low surrogate": GOOD.replace(b"awesome!", b"awe\\udc00some"),
        "a float": GOOD.replace(b'"view":12', b'"view":12.0'),
        "a negative number": GOOD.replace(b'"view":12', b'"view":-1'),
        "a leading zero": GOOD.replace(b'"view":12', b'"view":012'),
        "a missing field": GOOD.replace(b'"timestamp":34,', b""),
        "no signature": GOOD.replace(b',"signature":"' + sig + b'"', b""),
        "a raw control character": GOOD.replace(b"awesome!", b"awe\nsome"),
        "invalid UTF-8": GOOD.replace(b"awesome!", b"awe\xffsome"),
        "an array": b"[" + GOOD + b"]",
        "cut short": GOOD[:-1],
        "empty": b"",
    }
    for name, t in bad.items():
        assert wire.decode_reply_json(t) is None, name
    lib = wire.load()
    out = np.zeros(1, wire.ReplyHead)
    assert lib.pbft_wire_decode_reply_json(None, 5, out.ctypes.data, None, 0) == -1
    assert lib.pbft_wire_decode_reply_json(GOOD, len(GOOD), None, None, 0) == -1
    assert lib.pbft_wire_decode_reply_json(GOOD, len(GOOD), out.ctypes.data, None, 0) == -1  # no room for the result
    assert not out.view(np.uint8).any()


def test_reader_whitespace_field_order_unknown_fields_and_escapes():
    sig = bytes(range(64)).hex().encode()
    f = {"view": b'"view":12', "timestamp": b'"timestamp":34', "peer_id": b'"peer_id":"' + PID + b'"',
         "result": b'"result":"awesome!"', "replica": b'"replica":5', "signature": b'"signature":"' + sig + b'"'}
    rng = np.random.default_rng(11)
    for _ in range(40):
        keys = list(f)
        rng.shuffle(keys)
        ws = [b"", b" ", b"\n", b"\t \r\n"]
        parts = [f[k].replace(b":", ws[rng.integers(4)] + b":" + ws[rng.integers(4)], 1) for k in keys]
        parts.insert(int(rng.integers(len(parts) + 1)), b'"extra":{"a":[1,2.5e3,"x\\"y",null,true],"result":"no"}')
        t = ws[rng.integers(4)] + b"{" + (ws[rng.integers(4)] + b"," + ws[rng.integers(4)]).join(parts) + b"}" + ws[rng.integers(4)]
        assert check_against_json(t), t
        h, res = wire.decode_reply_json(t)
        assert res == b"awesome!" and int(h["status"]) == wire.RH_GENERAL and int(h["replica"]) == 5
    esc = {b'a\\"b': b'a"b', b"a\\\\b": b"a\\b", b"a\\/b": b"a/b", b"\\b\\f\\n\\r\\t": b"\b\f\n\r\t",
           b"\\u00e9\\u0041": "éA".encode(), b"\\ud83d\\ude00": "\U0001F600".encode(), b"\\u0000": b"\0"}
    for raw, want in esc.items():
        t = GOOD.replace(b"awesome!", raw)
        assert check_against_json(t)
        h, res = wire.decode_reply_json(t)
        assert res == want and t[int(h["result_off"]):int(h["result_off"]) + int(h["result_len"])] == raw
    # an escaped key and an escaped peer id are serde's too
    t = GOOD.replace(b'"view"', b'"vie\\u0077"').replace(PID, b"\\u0031" + PID[1:])
    assert PID[:1] == b"1" and check_against_json(t)


# ---- the model ----
def test_model_on_hand_checked_cases():
    w = A.world()
    mk = lambda s, ts, res, ci=0, **kw: A.reply(w, s, 1, ts, ci, res, **kw)  # noqa: E731
    texts = [mk(0, 7, b"r", forge=True),   # 0: forged: OK by its text, bit 0
             mk(1, 7, b"r"),               # 1
             mk(2, 7, b"r"),               # 2: (7, r) has signers {1, 2}: accepted, first = 1
             mk(3, 8, b"s"),               # 3: alone: not accepted
             mk(3, 8, b"s"),               # 4: the same again: counts once
             mk(0, 9, b"t", claim=1),      # 5: ESIGNER
             mk(0, 9, b"t"),               # 6: ECLIENT below
             mk(1, 7, b"r", ci=1),         # 7: another client: another envelope
             mk(1, 9, b'q"uote'),          # 8: general
             b"{}"]                        # 9
    ci = [0, 0, 0, 0, 0, 0, 5, 1, 0, 0]
    m = accept_reference(texts, A.CLIENTS, w.pids, 2, 8, w.verify, client_idx=ci)
    assert [int(s) for s in m["heads"]["status"]] == [0, 0, 0, 0, 0, wire.ACCEPT_ESIGNER, wire.ACCEPT_ECLIENT, 0,
                                                       wire.ACCEPT_OK | wire.ACCEPT_ESCAPED, wire.ACCEPT_EJSON]
    assert list(m["bits"]) == [False, True, True, True, True, False, False, True, True, False]
    N = wire.ACCEPT_NO_REPLY
    assert list(m["env_idx"]) == [0, 0, 0, 1, 1, N, N, 2, 3, N] and list(m["n_env"]) == [4, 0]
    assert list(m["counts"]) == [2, 1, 1, 1, 0, 0, 0, 0] and list(m["signers"][:4, 0]) == [0b110, 0b1000, 0b10, 0b10]
    c = m["certs"]
    assert [tuple(int(x) for x in c[e]) for e in range(4)] == [(1, 7, 1, 2, 0, 1), (1, 8, 3, 1, 0, 0), (1, 7, 7, 1, 1, 0),
                                                               (1, 9, 8, 1, 0, 0)]
    assert all(tuple(int(x) for x in c[e]) == (0, 0, N, 0, 0, 0) for e in range(4, 8))
    assert m["results"][8] == b'q"uote' and m["envelopes"][0].tobytes() == A.envelope(1, 7, A.CLIENTS[0], b"r")
    h8 = m["heads"][8]
    assert texts[8][int(h8["result_off"]):int(h8["result_off"]) + int(h8["result_len"])] == b'q\\"uote'
    # the device form defers what is not canonical; a short table loses the later envelopes and never miscounts
    d = accept_reference(texts, A.CLIENTS, w.pids, 2, 2, w.verify, client_idx=ci, settle=False)
    assert [int(s) for s in d["heads"]["status"]][8:] == [wire.ACCEPT_EDEFER] * 2
    assert list(d["env_idx"]) == [0, 0, 0, 1, 1, N, N, N, N, N] and list(d["n_env"]) == [3, 1]
    assert list(d["counts"]) == [2, 1] and int(d["certs"][0]["accepted"]) == 1
    # need = 1: a single valid reply decides; an empty batch
    assert list(accept_reference(texts, A.CLIENTS, w.pids, 1, 8, w.verify, client_idx=ci)["certs"]["accepted"][:4]) == [1] * 4
    e = accept_reference([], A.CLIENTS, w.pids, 2, 3, w.verify)
    assert list(e["n_env"]) == [0, 0] and list(e["certs"]["first"]) == [N] * 3


@pytest.mark.parametrize("n_honest,outside,settle", [(17, True, False), (85, False, True)])
def test_corpus_conditions(n_honest, outside, settle):
    """From the model alone: every status at least twice, at least 10 accepted envelopes and 5 that are not, and an
    accepted envelope whose first valid reply is not its first reply."""
    c = A.corpus(n_honest, with_outside=outside)
    n = len(c["texts"])
    assert n == 130 if n_honest == 17 else 380 <= n <= 420
    m = A.model(c, settle)
    st = [int(s) & 0xFF for s in m["heads"]["status"]]
    want = {wire.ACCEPT_OK, wire.ACCEPT_ESIGNER, wire.ACCEPT_ECLIENT, wire.ACCEPT_EJSON if settle else wire.ACCEPT_EDEFER}
    assert set(st) == want and all(st.count(s) >= 2 for s in want)
    ne = int(m["n_env"][0])
    acc = m["certs"]["accepted"][:ne].astype(bool)
    assert int(acc.sum()) >= 10 and int((~acc).sum()) >= 5
    firsts = [int(np.nonzero(m["env_idx"] == e)[0][0]) for e in range(ne)]
    assert any(acc[e] and int(m["certs"][e]["first"]) != firsts[e] for e in range(ne))
    lens = {len(r) for r, s in zip(m["results"], st) if s == 0}
    assert lens >= set(A.RES_LENS)
    if settle:
        assert sum(1 for s in m["heads"]["status"] if int(s) & wire.ACCEPT_ESCAPED) >= 8
    notes = set(c["note"])
    assert {"forged", "flipped", "wrong index", "wrong peer id", "replica 4", "replica 65535", "client 3", "twice",
            "equivocation", "two clients", "one answer", "two answers", "general", "cut short"} <= notes
    assert sum(x.startswith("near miss") for x in c["note"]) == 15 and ("outside" in notes) == outside


# ---- the stand-alone sanitizer run ----
NATIVE = os.path.join(ROOT, "tests", "native")
BIN = os.path.join(NATIVE, "accept_main")
CSRC = os.path.join(ROOT, "pbft_amd", "csrc")
SRCS = [os.path.join(NATIVE, "accept_main.cpp"), os.path.join(CSRC, "host", "wire.cpp")]
DEPS = SRCS + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + \
       [os.path.join(ROOT, "include", f) for f in os.listdir(os.path.join(ROOT, "include"))]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]


def test_parser_and_rule_clean_under_asan_ubsan(tmp_path):
    if not (os.path.exists(BIN) and all(os.path.getmtime(d) <= os.path.getmtime(BIN) for d in DEPS)):
        if not os.path.exists(HIPCC):
            pytest.skip("hipcc not present")
        subprocess.run([HIPCC, "--offload-host-only", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-pthread"] +
                       SAN + ["-o", BIN] + SRCS, check=True, timeout=900)
    c = A.corpus(17, with_outside=False)
    w = A.world()
    # the corpus as a file: the four PeerId texts, the clients' fields, then (client_idx, length, text) per reply
    blob = b"".join(w.pids) + b"".join(wire.client_field(x) for x in A.CLIENTS)
    for t, ci in zip(c["texts"], c["client_idx"]):
        blob += int(ci).to_bytes(4, "little") + len(t).to_bytes(4, "little") + t
    path = tmp_path / "corpus.bin"
    path.write_bytes(blob)
    env = dict(os.environ)
    sym = "/opt/rocm/lib/llvm/bin/llvm-symbolizer"
    if os.path.exists(sym):
        env["ASAN_SYMBOLIZER_PATH"] = sym
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0:halt_on_error=1"
    p = subprocess.run([BIN, str(path)], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    m = re.search(r"accept host run ok: (\d+) texts, (\d+) canonical, (\d+) parsed, (\d+) variants", p.stdout)
    assert m and int(m.group(1)) == len(c["texts"]) and int(m.group(4)) > 20000
    mod = A.model(c, settle=True)
    st = [int(s) & 0xFF for s in mod["heads"]["status"]]
    assert int(m.group(3)) == sum(s != wire.ACCEPT_EJSON for s in st)
    dev = A.model(c, settle=False)
    assert int(m.group(2)) == sum(int(s) != wire.ACCEPT_EDEFER for s in dev["heads"]["status"])
