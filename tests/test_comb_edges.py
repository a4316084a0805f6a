"""The edge-digit fixture tests/golden/comb_edges.npz proves its own coverage (CPU only).

The fixture's rows are valid signatures whose comb digits sit on the table edges of the production plans
(tests/comb_edges.py, tests/golden/gen_comb_edges.py).  Here: the model's plans are the ones verify_kernels.h
compiles, every row's tag is recomputed from its bytes, every target of every plan is present, and the expected bits
are those of both oracles."""
import ctypes
import hashlib
import os
import random
import re

import numpy as np
import pytest

import comb_edges as ce
import ed25519_ref as ref
from conftest import ROOT


@pytest.fixture(scope="module")
def fx():
    return ce.load()


def test_model_plans_are_the_compiled_ones():
    src = open(os.path.join(ROOT, "pbft_amd", "csrc", "verify_kernels.h")).read()
    ints = lambda s: tuple(int(x) for x in s.split(","))  # noqa: E731
    defs = {m.group(1): ints(m.group(2)) for m in re.finditer(r"#define (PBFT_PLAN_[AB]) ([\d, ]+)\n", src)}
    plans = {}
    for m in re.finditer(r"using (PL\w+) = plan<([^>]+)>;", src):
        plans[m.group(1)] = defs[m.group(2)] if m.group(2) in defs else ints(m.group(2))
    assert plans == {"PLB": ce.PLAN_B, "PLA_HUGE": ce.KEY_PLANS[13], "PLA_BIG": ce.KEY_PLANS[14],
                     "PLA_MID": ce.KEY_PLANS[16], "PLA_SMALL": ce.KEY_PLANS[32]}
    for pid, (p, w, nb) in ce.PLANS.items():
        assert p * w + nb == 254 and (pid == 0 or pid == p)
        assert ce.bitoff((p, w, nb), p - 1) + ce.width((p, w, nb), p - 1) == 254
        assert len(ce.all_targets(pid)) == ce.COUNTS[pid] == 6 * (p - 1) + 2


def test_recode_is_a_signed_digit_expansion():
    """The model's digits rebuild the scalar, stay in range, and reach the edges where the windows say so."""
    rnd = random.Random(1)
    for plan in ce.PLANS.values():
        p = plan[0]
        xs = [0, 1, ce.L - 1, (1 << 252) - 1, 1 << 252] + [rnd.randrange(ce.L) for _ in range(200)]
        for pos in range(p - 1):      # a window of all ones below a set bit: digit -1 here ... carries upwards
            xs.append(((1 << ce.width(plan, pos)) - 1) << ce.bitoff(plan, pos))
            xs.append(1 << (ce.bitoff(plan, pos) + ce.width(plan, pos) - 1))   # exactly half: the last entry, negated
        for x in xs:
            d = ce.recode(x, plan)
            assert sum(v << ce.bitoff(plan, i) for i, v in enumerate(d)) == x
            for i, v in enumerate(d[:-1]):
                h = 1 << (ce.width(plan, i) - 1)
                assert -h <= v < h
            assert 0 <= d[-1] <= 1 << (ce.width(plan, p - 1) - 1)
        pos = 0
        assert ce.recode(1 << (ce.width(plan, pos) - 1), plan)[:2] == [-(1 << (ce.width(plan, pos) - 1)), 1]


def test_every_tag_and_full_coverage(fx):
    n = len(fx["S"])
    assert n % 64 and n == 2 * sum(ce.COUNTS.values())
    key = fx["key"].tobytes()
    assert key == ref.public_key(fx["seed"].tobytes())
    seen = set()
    for i in range(n):
        R, S, M = fx["R"][i].tobytes(), fx["S"][i].tobytes(), fx["msg"][i].tobytes()
        pid, pos, tg = int(fx["plan"][i]), int(fx["pos"][i]), int(fx["target"][i])
        plan = ce.PLANS[pid]
        assert M[:4] == b"PBFT" and M[4] in (1, 2) and len(M) == 85
        s = int.from_bytes(S, "little")
        k = int.from_bytes(hashlib.sha512(R + key + M).digest(), "little") % ce.L
        assert s < ce.L
        if not fx["twin"][i]:
            assert fx["expected"][i] == 1
            assert ce.recode(s if pid == 0 else k, plan)[pos] == tg, (pid, pos, tg)
            assert tg in ce.targets(plan, pos)
            assert (pid, pos, tg) not in seen
            seen.add((pid, pos, tg))
        else:  # the row before it, one unit of the tagged position away
            assert fx["expected"][i] == 0 and not fx["twin"][i - 1]
            assert (R, M, pid, pos, tg) == (fx["R"][i - 1].tobytes(), fx["msg"][i - 1].tobytes(),
                                            int(fx["plan"][i - 1]), int(fx["pos"][i - 1]), int(fx["target"][i - 1]))
            s1 = int.from_bytes(fx["S"][i - 1].tobytes(), "little")
            assert abs(s - s1) == 1 << ce.bitoff(plan, pos)
            if pid == 0:
                assert abs(ce.recode(s, plan)[pos] - tg) == 1
    for pid, cnt in ce.COUNTS.items():
        want = set(ce.all_targets(pid))
        assert len(want) == cnt and {t for t in seen if t[0] == pid} == want, pid
    assert len(seen) == sum(ce.COUNTS.values())


def test_signer_set_tags_and_coverage(fx):
    seed = fx["sg_seed"].tobytes()
    _, prefix = ref.secret_expand(seed)
    assert fx["sg_pub"].tobytes() == ref.public_key(seed)
    seen = set()
    for i in range(len(fx["sg_msg"])):
        M = fx["sg_msg"][i].tobytes()
        assert M[:4] == b"PBFT" and M[4] in (1, 2) and len(M) == 85
        r = int.from_bytes(hashlib.sha512(prefix + M).digest(), "little") % ce.L
        pos, tg = int(fx["sg_pos"][i]), int(fx["sg_target"][i])
        assert ce.recode(r, ce.PLAN_B)[pos] == tg
        seen.add((pos, tg))
        sig = ref.sign(seed, M)
        assert sig == fx["sg_R"][i].tobytes() + fx["sg_S"][i].tobytes()
    assert seen == {(pos, tg) for pos in range(ce.PLAN_B[0]) for tg in ce.signer_targets(pos)}
    assert len(seen) == ce.SIGNER_COUNT == len(fx["sg_msg"])


def test_both_oracles_agree_on_every_row_and_twin(fx):
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))
    vp = ctypes.c_void_p
    lib.oracle_verify_batch.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32,
                                        ctypes.c_uint64, vp, ctypes.c_int]
    n = len(fx["S"])
    keys = np.ascontiguousarray(fx["key"].reshape(1, 32))
    R, S = np.ascontiguousarray(fx["R"]), np.ascontiguousarray(fx["S"])
    kidx, out = np.zeros(n, np.uint16), np.zeros(n, np.uint8)
    buf = np.zeros(n * 85 + 16, np.uint8)
    buf[: n * 85] = fx["msg"].reshape(-1)
    assert lib.oracle_verify_batch(keys.ctypes.data, 1, R.ctypes.data, S.ctypes.data, kidx.ctypes.data,
                                   buf.ctypes.data, 85, 85, n, out.ctypes.data, 4) == 0
    assert (out == fx["expected"]).all(), np.nonzero(out != fx["expected"])[0][:8]
    key = fx["key"].tobytes()
    py = [ref.verify_strict(key, fx["R"][i].tobytes() + fx["S"][i].tobytes(), fx["msg"][i].tobytes())
          for i in range(n)]
    assert (np.array(py, np.uint8) == fx["expected"]).all()
    assert (fx["expected"] == 1 - fx["twin"]).all()
