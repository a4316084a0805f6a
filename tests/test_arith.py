"""The field, scalar and comb-step arithmetic on raw limbs at its documented bounds, host build.

Every op of pbft_amd/csrc/debug_arith_core.h runs through hh_arith (tests/native/arith_harness.cpp, the op table
compiled for the host; built here when it is missing or older than its sources) on the cases of
tests/arith_cases.py -- every operand with its limbs at and around its role's bound, which no signature ever
produces -- and is compared exactly with Python integers: values mod p (mod L), output limbs within their stated
bounds, fe_mul_chain<N> limb for limb equal to fe_mul, the three forms of ge_madd_ab limb for limb equal.
tests/test_gpu_arith.py runs the same bodies on the gfx950 build.
"""
import ctypes
import os
import subprocess

import pytest

import arith_cases as A
from conftest import ROOT


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(ROOT, "tests", "native", "arith_harness.cpp")
LIB = os.path.join(ROOT, "tests", "native", "libarith_harness.so")
CSRC = os.path.join(ROOT, "pbft_amd", "csrc")


def build_harness():
    deps = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if os.path.exists(LIB) and all(os.path.getmtime(d) <= os.path.getmtime(LIB) for d in deps):
        return LIB
    subprocess.run([HIPCC, "--offload-host-only", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC],
                   check=True, timeout=600)
    return LIB


class HostBackend:
    def __init__(self):
        lib = ctypes.CDLL(build_harness())
        vp = ctypes.c_void_p
        lib.hh_arith.argtypes = [ctypes.c_int, vp, vp, ctypes.c_uint32]
        lib.hh_arith_info.argtypes = [ctypes.c_int, vp, vp, vp]
        self.lib = lib
        self.ops = A.read_ops(lib.hh_arith_info)
        self.results = {}

    def call(self, op, inp, out, n):
        return self.lib.hh_arith(op, None if inp is None else inp.ctypes.data,
                                 None if out is None else out.ctypes.data, n)


@pytest.fixture(scope="module")
def be():
    return HostBackend()


def test_op_table_matches_the_cases(be):
    assert sorted(be.ops) == sorted(n for g in A.GROUPS.values() for n in g)
    for name in be.ops:
        assert A.cases(name).shape[1] == be.ops[name][1], name
        assert 0 < len(A.cases(name)) <= A.MAX_ITEMS, name


def test_every_op_has_all_maximum_operands():
    A.check_all_maximum_everywhere()


@pytest.mark.parametrize("group", sorted(A.GROUPS))
def test_group(be, group):
    A.CHECKS[group](be)


def test_hook_edges(be):
    A.check_hook_edges(be)
