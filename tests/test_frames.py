"""The frame decoder without a GPU: the parse core every GPU lane runs (pbft_amd/csrc/wire_decode_core.h) built for the
host into a stand-alone program (tests/native/frames_main.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer and
compared with the host's own parser; pbft_wire_frame_index; and the Python surface."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NATIVE = os.path.join(ROOT, "tests", "native")
BIN = os.path.join(NATIVE, "frames_main")
SRCS = [os.path.join(NATIVE, "frames_main.cpp"), os.path.join(ROOT, "pbft_amd", "csrc", "host", "wire.cpp")]
DEPS = SRCS + [os.path.join(ROOT, "pbft_amd", "csrc", "wire_decode_core.h")] + \
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


def test_core_matches_host_parser_under_asan_ubsan():
    """>= 20,000 canonical frames (never deferred, ESIGNER exactly by the signer rule, records and heads equal to
    pbft_records_pack of the host parser's fields) and >= 50,000 mutated ones (the core accepts exactly the bodies that
    the general parser reads as a signed vote and writes back byte for byte), each in a heap buffer of its own length;
    pbft_wire_frame_index against the framing of pbft_wire_decode_votes."""
    _build()
    env = dict(os.environ)
    sym = "/opt/rocm/lib/llvm/bin/llvm-symbolizer"
    if os.path.exists(sym):
        env["ASAN_SYMBOLIZER_PATH"] = sym
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0:halt_on_error=1"
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    assert "frames host run ok" in p.stdout
    assert int(re.search(r"canonical frames: (\d+)", p.stdout).group(1)) >= 20000
    m = re.search(r"mutated frames: (\d+) \((\d+) canonical, (\d+) valid", p.stdout)
    mutated, accepted, valid = (int(x) for x in m.groups())
    assert mutated >= 50000
    assert 0 < accepted < valid < mutated  # all three kinds of outcome occur among the mutants
    assert int(re.search(r"indexed streams: (\d+)", p.stdout).group(1)) >= 400


def _votes(n, seed=0):
    rng = np.random.default_rng(seed)
    kind = rng.integers(1, 3, n).astype(np.uint8)
    view = rng.integers(0, 2**63, n).astype(np.uint64) >> rng.integers(0, 63, n).astype(np.uint64)
    seq = rng.integers(0, 2**63, n).astype(np.uint64) >> rng.integers(0, 63, n).astype(np.uint64)
    dig, sig = rng.integers(0, 256, (n, 64), dtype=np.uint8), rng.integers(0, 256, (n, 64), dtype=np.uint8)
    rep = rng.integers(0, 300, n).astype(np.uint32)
    return kind, view, seq, dig, rep, sig


def test_symbols_exported():
    import pbft_amd
    lib = pbft_amd.load()
    for f in ("pbft_wire_frame_index", "pbft_wire_decode_frames_device", "pbft_verify_frames_device",
              "pbft_verify_frames"):
        assert hasattr(lib, f) and f in pbft_amd.EXPORTS
    assert pbft_amd.FrameHead.itemsize == 24
    assert [pbft_amd.FrameHead.fields[k][1] for k in ("view", "seq", "key_idx", "kind", "status", "frame_len")] == \
           [0, 8, 16, 18, 19, 20]


def test_frame_index_round_trips_encode_votes():
    from pbft_amd import frame_index, wire
    kind, view, seq, dig, rep, sig = _votes(200, 1)
    stream = wire.encode_votes(kind, view, seq, dig, rep, sig)
    off, flen, used = frame_index(stream)
    assert len(off) == 200 and used == len(stream)
    assert flen.min() >= wire.FRAME_MIN and flen.max() <= wire.FRAME_MAX
    for f in range(200):
        m = wire.decode_json(stream[off[f]: off[f] + flen[f]].tobytes())
        assert (m.kind, m.view, m.seq, m.replica) == (kind[f], view[f], seq[f], rep[f])
        assert m.digest == dig[f].tobytes() and m.sig == sig[f].tobytes()
    assert (off[1:] == off[:-1] + flen[:-1] + 2).all()  # (a two-byte varint in front of each 336..379-byte body)
    # an incomplete last frame stays; the framing is that of decode_votes
    cut = stream[: len(stream) - 7]
    off2, flen2, used2 = frame_index(cut)
    v = wire.decode_votes(cut.tobytes(), 300)
    assert len(off2) == 199 == len(v.status) and used2 == v.consumed == off[199] - 2
    assert (off2 == off[:199]).all() and (flen2 == flen[:199]).all()
    assert frame_index(stream, max_frames=5)[2] == off[5] - 2
    assert frame_index(b"")[2] == 0 and len(frame_index(b"")[0]) == 0
    with pytest.raises(pbft_error()):
        frame_index(bytes([0x80, 0x00]) + cut.tobytes())  # non-minimal varint


def pbft_error():
    from pbft_amd import PbftError
    return PbftError


def test_null_and_range_arguments_are_errors():
    import pbft_amd
    lib = pbft_amd.load()
    assert lib.pbft_verify_frames(None, None, 0, None, None, None, 4, 0, None, None, None) == -1
    assert lib.pbft_verify_frames_device(None, None, 0, None, None, None, 4, 0, None, None, None, None) == -1
    assert lib.pbft_wire_decode_frames_device(None, None, 0, None, None, None, 4, 0, None, None, None) == -1
    assert lib.pbft_wire_frame_index(None, 0, 0, None, None, None, None) == -1


def test_verify_frames_needs_a_device():
    """No CPU path: without a gfx950 GPU the verifier that owns verify_frames does not come into being."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import pbft_amd
    kind, view, seq, dig, rep, sig = _votes(3, 2)
    stream = pbft_amd.wire.encode_votes(kind, view, seq, dig, rep, sig)
    off, flen, _ = pbft_amd.frame_index(stream)
    with pytest.raises(pbft_amd.PbftError) as e:
        pbft_amd.GpuBatchVerifier(0).verify_frames(stream, off, flen)
    assert e.value.code == -5  # PBFT_ENODEV
