"""The pure-host half of the blocking signing forms without a GPU: the staging layout, the item span check and the merge
of device-written and general items (pbft_amd/csrc/sign_host.h) as a stand-alone program under AddressSanitizer + UBSan,
linked with the host encoders (tests/native/sign_host_main.cpp)."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

NATIVE = os.path.join(ROOT, "tests", "native")
BIN = os.path.join(NATIVE, "sign_host_main")
CSRC = os.path.join(ROOT, "pbft_amd", "csrc")
SRCS = [os.path.join(NATIVE, "sign_host_main.cpp"), os.path.join(CSRC, "host", "wire.cpp")]
DEPS = SRCS + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + \
       [os.path.join(ROOT, "include", f) for f in os.listdir(os.path.join(ROOT, "include"))]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]


def test_layout_span_check_and_merge_clean_under_asan_ubsan():
    if not (os.path.exists(BIN) and all(os.path.getmtime(d) <= os.path.getmtime(BIN) for d in DEPS)):
        if not os.path.exists(HIPCC):
            pytest.skip("hipcc not present")
        subprocess.run([HIPCC, "--offload-host-only", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer"] + SAN +
                       ["-o", BIN] + SRCS, check=True, timeout=900)
    env = dict(os.environ)
    sym = "/opt/rocm/lib/llvm/bin/llvm-symbolizer"
    if os.path.exists(sym):
        env["ASAN_SYMBOLIZER_PATH"] = sym
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0:halt_on_error=1"
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    m = re.search(r"sign host run ok: (\d+) layouts, (\d+) merges", p.stdout)
    assert m and int(m.group(1)) >= 150 and int(m.group(2)) >= 10
