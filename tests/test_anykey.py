"""Verification under uninstalled keys without a GPU: anykey_core.h's host build as a stand-alone program under
AddressSanitizer + UBSan (tests/native/anykey_main.cpp) on the golden corpus with every key carried inline and on the
point hook's (s, k, A) triples against oracle/ed25519_ref.py; the inputs' digit coverage; the entry points' null
arguments."""
import os
import re
import subprocess

import numpy as np
import pytest

import anykey_cases as C
from conftest import ROOT

NATIVE = os.path.join(ROOT, "tests", "native")
BIN = os.path.join(NATIVE, "anykey_main")
CSRC = os.path.join(ROOT, "pbft_amd", "csrc")
SRCS = [os.path.join(NATIVE, "anykey_main.cpp")]
DEPS = SRCS + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def program():
    if not (os.path.exists(BIN) and all(os.path.getmtime(d) <= os.path.getmtime(BIN) for d in DEPS)):
        if not os.path.exists(HIPCC):
            pytest.skip("hipcc not present")
        subprocess.run([HIPCC, "--offload-host-only", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer"] + SAN +
                       ["-o", BIN] + SRCS, check=True, timeout=900)
    return BIN


def run_program(program, tmp_path, records):
    """records: [(mode, n, msg_len, msg_stride, [arrays])] -> the program's output bytes"""
    blob = b""
    for mode, n, msg_len, msg_stride, arrays in records:
        blob += np.array([mode, n, msg_len, msg_stride], "<u4").tobytes() + b"".join(a.tobytes() for a in arrays)
    src, dst = tmp_path / "cases.bin", tmp_path / "out.bin"
    src.write_bytes(blob)
    env = dict(os.environ)
    sym = "/opt/rocm/lib/llvm/bin/llvm-symbolizer"
    if os.path.exists(sym):
        env["ASAN_SYMBOLIZER_PATH"] = sym
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0:halt_on_error=1"
    p = subprocess.run([program, str(src), str(dst)], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    m = re.search(r"anykey host run ok: (\d+) records, (\d+) items", p.stdout)
    assert m and int(m.group(1)) == len(records) and int(m.group(2)) == sum(r[1] for r in records)
    return dst.read_bytes()


def test_golden_corpus_with_inline_keys(program, tmp_path):
    batches = C.golden_inline()
    assert len(batches) == 11 and sum(len(b[1]) for b in batches) == 2180
    out = run_program(program, tmp_path, [(0, len(R), ml, msg.shape[1], [R, S, A, msg]) for ml, R, S, A, msg, _ in batches])
    at = 0
    for ml, R, S, A, msg, exp in batches:
        got = np.frombuffer(out[at:at + len(R)], np.uint8).astype(bool)
        at += len(R)
        bad = np.nonzero(got != exp)[0]
        assert len(bad) == 0, (ml, bad[:10])
    assert at == len(out)


def test_point_hook_against_the_reference(program, tmp_path):
    s, k, A, enc, kok, dec = C.point_cases()
    n = len(s)
    out = run_program(program, tmp_path, [(1, n, 0, 0, [s, k, A])])
    assert len(out) == 33 * n
    got = np.frombuffer(out[:32 * n], np.uint8).reshape(n, 32)
    got_ok = np.frombuffer(out[32 * n:], np.uint8)
    assert (got_ok == kok).all(), np.nonzero(got_ok != kok)[0][:10]
    d = dec.astype(bool)
    bad = np.nonzero((got[d] != enc[d]).any(axis=1))[0]
    assert len(bad) == 0, bad[:10]
    assert 0 < int((kok == 0).sum()) < n and int((~d).sum()) == 1


def test_point_cases_reach_every_digit():
    at0, at62, top = C.check_digit_coverage()
    assert at0 == set(range(-8, 8)) and at62 == set(range(-8, 8)) and top == {0, 1, 2}
    # the issue's scalars: every nibble 8 recodes to -8 in every window but the last, every nibble 7 to 7
    assert C.recode(C.NIB8 % (1 << 252))[:62] == [-8] + [-7] * 61 and C.recode(int("7" * 63, 16))[:63] == [7] * 63
    assert C.recode((1 << 252) + (1 << 251))[62:] == [-8, 2]


def test_null_arguments():
    import pbft_amd
    lib = pbft_amd.load()
    for f in ("pbft_verify_batch_keys", "pbft_verify_batch_keys_device", "pbft_debug_anykey_point"):
        assert hasattr(lib, f)
    assert "pbft_verify_batch_keys" in pbft_amd.EXPORTS and "pbft_verify_batch_keys_device" in pbft_amd.EXPORTS
    assert lib.pbft_verify_batch_keys(None, None, None, None, None, 0, 0, 0, None) == -1
    assert lib.pbft_verify_batch_keys_device(None, None, None, None, None, 0, 0, 0, None, None) == -1
    assert lib.pbft_debug_anykey_point(None, None, None, None, 0, None, None) == -1
