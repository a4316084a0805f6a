"""The replica's admission rule without a GPU: the code every GPU lane runs (pbft_amd/csrc/admit_core.h: classify, key
planes, resolve, residue) built for the host into a stand-alone program (tests/native/admit_main.cpp) under
AddressSanitizer + UndefinedBehaviorSanitizer and compared with pbft_amd.admit_reference; and the Python surface."""
import os
import re
import subprocess

import numpy as np
import pytest

import admit_cases
from conftest import ROOT

NATIVE = os.path.join(ROOT, "tests", "native")
BIN = os.path.join(NATIVE, "admit_main")
SRCS = [os.path.join(NATIVE, "admit_main.cpp")]
DEPS = SRCS + [os.path.join(ROOT, "pbft_amd", "csrc", "admit_core.h")] + \
       [os.path.join(ROOT, "include", f) for f in os.listdir(os.path.join(ROOT, "include"))]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]


def _build():
    if os.path.exists(BIN) and all(os.path.getmtime(d) <= os.path.getmtime(BIN) for d in DEPS):
        return
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    cmd = [HIPCC, "--offload-host-only", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer"] + SAN + \
          ["-o", BIN] + SRCS
    subprocess.run(cmd, check=True, timeout=600)


def _run(cases, tmp_path):
    """Every case through the program: a list of dicts shaped like admit_reference's result."""
    _build()
    from pbft_amd.wire import AdmitResidue
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.uint64(len(cases)).tobytes())
        for c in cases:
            n = len(c["rows"])
            off, flen = admit_cases.index_of(n)
            f.write(np.array([n, n if c["n_total"] is None else c["n_total"], c["view"], c["h"], c["log_window"],
                              c["n_keys"], c["residue_cap"]], dtype=np.uint64).tobytes())
            f.write(admit_cases.to_heads(c["rows"]).tobytes())
            f.write(off.tobytes())
            f.write(flen.tobytes())
    env = dict(os.environ)
    sym = "/opt/rocm/lib/llvm/bin/llvm-symbolizer"
    if os.path.exists(sym):
        env["ASAN_SYMBOLIZER_PATH"] = sym
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0:halt_on_error=1"
    p = subprocess.run([BIN, src, dst], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    m = re.search(r"admit host run ok: (\d+) cases, (\d+) rows", p.stdout)
    assert m and int(m.group(1)) == len(cases)
    buf = open(dst, "rb").read()
    out, at = [], 0

    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(buf, dtype=dtype, count=count, offset=at)
        at += a.nbytes
        return a

    for c in cases:
        n = len(c["rows"])
        out.append(dict(cls=take(np.uint8, n), counts=take(np.uint32, 8), clean=take(np.uint64, (n + 63) // 64),
                        res=take(AdmitResidue, c["residue_cap"]), n_res=take(np.uint32, 2),
                        keep=take(np.uint8, n).astype(bool)))
    assert at == len(buf)
    return out


def _reference(c):
    import pbft_amd
    n = len(c["rows"])
    off, flen = admit_cases.index_of(n)
    return pbft_amd.admit_reference(admit_cases.to_heads(c["rows"]), c["view"], c["h"], c["log_window"], c["n_keys"],
                                    c["residue_cap"], n_total=c["n_total"], off=off, flen=flen)


def _same(got, want, name):
    for k in ("cls", "counts", "clean", "res", "n_res", "keep"):
        assert np.array_equal(got[k], want[k]), (name, k, got[k][:16], want[k][:16])


def test_host_build_matches_reference_under_asan_ubsan(tmp_path):
    """The case list of the admission pass -- both watermarks and one past each, a window that reaches past 2^64, a
    wrong view with a bad seq, every status value, one (seq, signer) under both kinds, pairs and triples of contested
    rows across wave and block boundaries, padding behind the total, a residue_cap below the residue, the largest key
    planes, and random mixtures of 1, 63, 64, 65 and 4099 rows -- gives the same class, counts, clean bitmap, residue
    list, totals and kept key indices in the program (rows marked in both orders) and in admit_reference."""
    cases = admit_cases.cases()
    for c, got in zip(cases, _run(cases, tmp_path)):
        _same(got, _reference(c), c["name"])


def test_reference_on_the_cases_by_hand():
    """admit_reference itself, against classes written down by hand."""
    import pbft_amd
    from pbft_amd import verifier as v
    by = {c["name"]: c for c in admit_cases.cases()}
    C, X, V, W, S, H, P = (v.ADMIT_CLEAN, v.ADMIT_CONTESTED, v.ADMIT_REJ_VIEW, v.ADMIT_REJ_WATERMARK,
                           v.ADMIT_REJ_SIGNER, v.ADMIT_HOST, v.ADMIT_PAD)
    assert list(_reference(by["watermarks"])["cls"]) == [W, C, C, W] * 2
    # h = 2^64 - 3, window 8: 2^64 - 2 and 2^64 - 1 are inside; 0, 1, 5 (wrapped) and 2^64 - 4 are not
    assert list(_reference(by["window past 2^64"])["cls"]) == [W, C, C, W, W, W, W, W, W]
    assert list(_reference(by["view before window"])["cls"]) == [V, V, V, W]
    assert list(_reference(by["every status"])["cls"]) == \
        [H, H, H, H, S, H, H, H] + [C, H, H, H, H, S, H, H] + [H, H, C, S, S, C]
    assert list(_reference(by["both kinds"])["cls"]) == [C, C, C, C]
    r = _reference(by["pairs"])
    assert list(np.flatnonzero(r["cls"] == X)) == [0, 1, 63, 64, 255, 256] and r["counts"][C] == 294
    assert list(r["res"]["frame"][:6]) == [0, 1, 63, 64, 255, 256] and list(r["n_res"]) == [6, 0]
    assert list(r["res"]["off"][:2]) == [1000, 1400] and list(r["res"]["len"][:2]) == [340, 341]
    assert not r["keep"][[0, 1, 63, 64, 255, 256]].any() and r["keep"].sum() == 294
    r = _reference(by["triples"])
    assert list(np.flatnonzero(r["cls"] == X)) == [0, 1, 2, 63, 64, 130, 255, 256, 299]
    r = _reference(by["pairs across kinds"])
    assert r["cls"][16] == C and list(r["cls"][:3]) == [X, X, C]
    r = _reference(by["padding"])
    assert (r["cls"][:66] == C).all() and (r["cls"][66:] == P).all() and list(r["n_res"]) == [0, 0]
    assert r["clean"][1] == 3
    assert (_reference(by["nothing valid"])["cls"] == P).all()
    r = _reference(by["residue cap"])
    assert list(r["n_res"]) == [9, 6] and list(r["res"]["frame"]) == [0, 1, 63]
    r = _reference(by["no residue room"])
    assert list(r["n_res"]) == [2, 2] and len(r["res"]) == 0
    assert list(_reference(by["largest window"])["cls"]) == [C, X, X, W]
    assert pbft_amd.admit_reference is v.admit_reference


def test_in_log_has_one_definition():
    """The replica's window test is admit_core.h's predicate: replica.cpp calls it and spells no second one."""
    src = open(os.path.join(ROOT, "pbft_amd", "csrc", "host", "replica.cpp")).read()
    assert "pbft::admit_in_log(r->h, r->log_window, seq)" in src
    assert "seq - r->h <= r->log_window" not in src
    core = open(os.path.join(ROOT, "pbft_amd", "csrc", "admit_core.h")).read()
    assert "return seq > h && seq - h <= log_window;" in core


def test_symbols_exported():
    import pbft_amd
    lib = pbft_amd.load()
    for f in ("pbft_admit_device", "pbft_admit_reserve"):
        assert hasattr(lib, f) and f in pbft_amd.EXPORTS
    assert pbft_amd.AdmitResidue.itemsize == 16
    assert [pbft_amd.AdmitResidue.fields[k][1] for k in ("off", "frame", "len")] == [0, 8, 12]
    for name in ("admit_device", "admit_reserve"):
        assert callable(getattr(pbft_amd.GpuBatchVerifier, name))
    hdr = open(os.path.join(ROOT, "include", "pbft_wire.h")).read()
    from pbft_amd import verifier as v
    for name in ("CLEAN", "CONTESTED", "REJ_VIEW", "REJ_WATERMARK", "REJ_SIGNER", "HOST", "PAD", "CLASSES"):
        assert int(re.search(rf"#define PBFT_ADMIT_{name} (\d+)\b", hdr).group(1)) == getattr(v, "ADMIT_" + name)


def test_null_and_range_arguments_are_errors():
    import pbft_amd
    lib = pbft_amd.load()
    assert lib.pbft_admit_device(None, None, None, None, None, None, 0, 1, 0, 8, 4, 0, None, None, None, None, None,
                                 None) == -1
    assert lib.pbft_admit_reserve(None, 8, 4, 0) == -1
