"""bench.py's command line: a plain run measures the headline only and can write the round's bitmap
(--dump-outputs); everything else the line reports is behind --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
# what only --full measures: labelled figures (None in a plain line) and the side legs (absent from it)
FULL_FIGURES = ("weak_scaling", "sequential_rounds", "cpu_baseline", "cpu_baseline_openssl", "vs_cpu_openssl")
FULL_LEGS = ("shard_of_8", "p50_ms_4k_round", "stream_4k", "replica_flush_2^20", "replica_ingress_2^20", "e2e_2^20",
             "config2", "config3", "shuffled_2^20", "c_abi_multi_1gpu", "key_plans_2^20", "rekey_ms")


def test_options_present_and_off_by_default():
    p = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "--full" in p.stdout and "--dump-outputs DIR" in p.stdout


@pytest.mark.gpu
def test_plain_run_is_the_headline_only_and_dumps_the_round_bitmap(tmp_path):
    """A small round (5 replicas x 7 seqs x 2 = 70 signatures: a partial last bitmap word), 3 timed steps."""
    import bench
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--replicas", "5",
                        "--seqs", "7", "--settle-s", "0", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    for k in HEADLINE:
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "verifies/s" and line["higher_is_better"] is True
    n = 2 * 5 * 7
    assert line["config"]["sigs_per_step"] == n
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - n / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    for k in FULL_FIGURES:
        assert line[k] is None, k
    for k in FULL_LEGS:
        assert k not in line, k
    assert sorted(os.listdir(out)) == ["round_valid.npy"]
    got = np.load(out / "round_valid.npy")
    assert got.dtype == np.float32 and got.shape == (n,)
    _, bad = bench.corrupt(np.zeros((n, 32), np.uint8), bench.ADV_FRAC, bench.SEED)  # the seeded corrupted positions
    expect = np.ones(n, np.float32)
    expect[bad] = 0
    assert (got == expect).all(), np.nonzero(got != expect)[0]
