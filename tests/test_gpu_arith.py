"""The field, scalar and comb-step arithmetic on raw limbs at its documented bounds, as compiled for gfx950.

The bodies and cases of tests/test_arith.py, run through the library's test hook pbft_debug_arith
(pbft_amd/csrc/debug_arith.hip): one launch per op, one item per lane.  This is where the device-only forms run on
chosen operands -- fe_mul_chain's column asm (mad_column10, with and without carry-in), dbl32, lane_mask, the
bit-selects of fe_cneg_canon and ge_from_ab, the device compile of sc_reduce512_fold.  The hook holds its own
instance of each function: it checks the source as the device compiler sees it; the round tests check the verify
kernels as compiled.
"""
import ctypes

import pytest

import arith_cases as A

pytestmark = pytest.mark.gpu


class GpuBackend:
    def __init__(self):
        from pbft_amd._lib import load
        lib = load()
        vp = ctypes.c_void_p
        lib.pbft_debug_arith.argtypes = [ctypes.c_int, vp, vp, ctypes.c_uint32]
        lib.pbft_debug_arith.restype = ctypes.c_int
        lib.pbft_debug_arith_info.argtypes = [ctypes.c_int, vp, vp, vp]
        lib.pbft_debug_arith_info.restype = ctypes.c_int
        self.lib = lib
        self.ops = A.read_ops(lib.pbft_debug_arith_info)
        self.results = {}

    def call(self, op, inp, out, n):
        return self.lib.pbft_debug_arith(op, None if inp is None else inp.ctypes.data,
                                         None if out is None else out.ctypes.data, n)


@pytest.fixture(scope="module")
def be():
    return GpuBackend()


def test_op_table_matches_the_cases(be):
    assert sorted(be.ops) == sorted(n for g in A.GROUPS.values() for n in g)
    for name in be.ops:
        assert A.cases(name).shape[1] == be.ops[name][1], name


@pytest.mark.parametrize("group", sorted(A.GROUPS))
def test_group(be, group):
    A.CHECKS[group](be)


def test_hook_edges(be):
    A.check_hook_edges(be)
