"""The stream index without a GPU: the scheme every GPU lane runs (pbft_amd/csrc/wire_index_core.h: step, tile tables,
composition, resolve, emit) built for the host into a stand-alone program (tests/native/index_main.cpp) under
AddressSanitizer + UndefinedBehaviorSanitizer and compared with pbft_wire_frame_index; and the Python surface."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NATIVE = os.path.join(ROOT, "tests", "native")
BIN = os.path.join(NATIVE, "index_main")
SRCS = [os.path.join(NATIVE, "index_main.cpp"), os.path.join(ROOT, "pbft_amd", "csrc", "host", "wire.cpp")]
DEPS = SRCS + [os.path.join(ROOT, "pbft_amd", "csrc", "wire_index_core.h")] + \
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


def test_scheme_matches_host_walk_under_asan_ubsan():
    """>= 2,000 streams of 1..9 segments, each segment in a heap buffer of exactly its length, at tile 512 and at the
    default (some at 2048 too): frame lengths 0, 1, 127, 128, 336..379, 16383, 16384 and ~70,000; cuts inside a varint,
    inside a body and on a boundary; tails 0x80 x 1..11, 0x80 0x00, a length of 2^27 and of 2^27 + 1; errors and stops
    mid-stream and with their varint on a tile's last bytes; segments outside the stream; frame_cap below and above
    the total.  Frames, lengths, offsets, peers, consumed, status, first and the totals equal pbft_wire_frame_index's
    per segment, and the padding is as specified."""
    _build()
    env = dict(os.environ)
    sym = "/opt/rocm/lib/llvm/bin/llvm-symbolizer"
    if os.path.exists(sym):
        env["ASAN_SYMBOLIZER_PATH"] = sym
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0:halt_on_error=1"
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    assert "index host run ok" in p.stdout
    m = re.search(r"indexed streams: (\d+) \((\d+) segments, (\d+) frames\)", p.stdout)
    streams, segments, frames = (int(x) for x in m.groups())
    assert streams >= 2000 and segments > streams and frames > 100000
    m = re.search(r"framing errors: (\d+), stops with frames behind: (\d+), on a tile edge: (\d+), outside: (\d+), "
                  r"capped: (\d+)", p.stdout)
    assert all(int(x) >= 20 for x in m.groups())


def test_symbols_exported():
    import pbft_amd
    lib = pbft_amd.load()
    for f in ("pbft_wire_index_streams_device", "pbft_index_reserve", "pbft_verify_streams_tally_device",
              "pbft_verify_streams_tally"):
        assert hasattr(lib, f) and f in pbft_amd.EXPORTS
    assert pbft_amd.SegHead.itemsize == 24
    assert [pbft_amd.SegHead.fields[k][1] for k in ("consumed", "first", "n_frames", "status", "pad")] == \
           [0, 8, 12, 16, 20]
    for name in ("index_streams_device", "index_reserve", "verify_streams_tally_device", "verify_streams_tally"):
        assert callable(getattr(pbft_amd.GpuBatchVerifier, name))


def test_option_number_is_one_everywhere():
    """PBFT_OPT_INDEX_TILE has one number in the C header, the Python binding and the Rust crate, and no other option
    has it."""
    hdr = open(os.path.join(ROOT, "include", "pbft_verify.h")).read()
    num = int(re.search(r"#define PBFT_OPT_INDEX_TILE (\d+)\b", hdr).group(1))
    others = [int(x) for x in re.findall(r"#define PBFT_OPT_\w+ (\d+)\b", hdr)]
    assert others.count(num) == 1 and num == max(others)
    import pbft_amd
    assert pbft_amd.GpuBatchVerifier.OPT_INDEX_TILE == num
    assert re.search(rf"pub const PBFT_OPT_INDEX_TILE: c_int = {num};",
                     open(os.path.join(ROOT, "pbft-hip", "src", "ffi.rs")).read())
    assert "case PBFT_OPT_INDEX_TILE:" in open(os.path.join(ROOT, "pbft_amd", "csrc", "pbft_verify.hip")).read()


def test_null_and_range_arguments_are_errors():
    import pbft_amd
    lib = pbft_amd.load()
    assert lib.pbft_wire_index_streams_device(None, None, 0, None, None, None, 0, 0, None, None, None, None, None,
                                              None) == -1
    assert lib.pbft_index_reserve(None, 0, 0) == -1
    assert lib.pbft_verify_streams_tally_device(None, None, 0, None, None, None, 0, 4, 0, None, None, None, None, None,
                                                None, None, None, 0, None, None, None, None, None, None) == -1
    assert lib.pbft_verify_streams_tally(None, None, 0, None, None, None, 0, 4, 0, 0, None, None, None, None, None,
                                         None, None, None, None, None, None) == -1
    assert lib.pbft_verify_set_option(None, 19, 512) == -1


def test_streams_tally_needs_a_device():
    """No CPU path: without a gfx950 GPU the verifier that owns verify_streams_tally (and the PBFT_OPT_INDEX_TILE
    option) does not come into being."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import pbft_amd
    with pytest.raises(pbft_amd.PbftError) as e:
        pbft_amd.GpuBatchVerifier(0).verify_streams_tally(np.zeros(16, np.uint8), [0], [16], 4, 4)
    assert e.value.code == -5  # PBFT_ENODEV
