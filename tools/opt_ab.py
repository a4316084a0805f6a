#!/usr/bin/env python3
"""Interleaved A/B of one pbft_verify_set_option on ONE context (same tables, same process), device-resident
launches of the config-#4 round's first n signatures (comb + finish per launch), per size.

Value A runs as two of the three interleaved variants (A and A'), so every round also times A against itself: the
run-to-run spread is the median over the rounds of |A' - A| / A (its largest value is printed too), and the delta
of B is judged against that, as the difference of the medians and as the median of the per-round differences.
usage: python tools/opt_ab.py OPTION VALUE_A VALUE_B [--sizes 131072,65536] [--rounds 8] [--iters 20]
e.g. tools/opt_ab.py 13 0 1   (PBFT_OPT_COMB_PRIO off / on)"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("option", type=int)
    ap.add_argument("a", type=int)
    ap.add_argument("b", type=int)
    ap.add_argument("--sizes", default="131072,65536,262144,1048576")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    import torch
    import bench
    from pbft_amd import GpuBatchVerifier, bitmap_to_bool
    torch.cuda.set_device(0)
    seeds = bench.key_seeds(256)
    msg, key_idx = bench.envelopes(1, 2048, 256)
    v = GpuBatchVerifier(0)
    R, S, pub = v.sign(seeds, key_idx, msg, 85)
    assert v.set_keys(pub).all()
    dev = torch.device("cuda", 0)
    d = bench.to_device(torch, dev, R, S, key_idx, msg)
    st = torch.cuda.Stream(dev)
    for n in [int(x) for x in a.sizes.split(",")]:
        # three interleaved variants: A, A again (its distance from A is the run-to-run spread), B
        names = ("A", "A'", "B")
        val = {"A": a.a, "A'": a.a, "B": a.b}
        t = {k: [] for k in names}
        bits = {}
        for r in range(a.rounds):
            for k in names[r % 3:] + names[:r % 3]:
                v.set_option(a.option, val[k])
                ms, _ = bench.time_device(v, st, d, n, 3, torch)  # settle after the switch
                ms, _ = bench.time_device(v, st, d, n, a.iters, torch)
                t[k].append(ms)
                bits[k] = d["B"][: (n + 63) // 64].cpu().numpy().copy()
        assert (bits["A"] == bits["B"]).all() and bitmap_to_bool(bits["A"].view(np.uint64), n).all(), n
        med = {k: float(np.median(t[k])) for k in names}
        ta, ta2, tb = (np.array(t[k]) for k in names)
        aa = 100 * np.abs(ta2 - ta) / ta          # per round: A against itself
        ba = 100 * (tb - ta) / ta                 # per round: B against A
        spread = float(np.median(aa))
        delta = 100 * (med["B"] - med["A"]) / med["A"]
        print(f"n={n:8d} option {a.option}: " + "   ".join(
            f"{k} (={val[k]}) median {med[k]:.4f} ms min {min(t[k]):.4f}" for k in names)
            + f"   per-round |A'-A| median {spread:.2f} % max {aa.max():.2f} %   B-A delta of medians {delta:+.2f} % "
            f"({abs(delta) / max(spread, 1e-9):.1f} x spread), per round median {np.median(ba):+.2f} % "
            f"[{ba.min():+.2f} .. {ba.max():+.2f}], B faster in {int((ba < 0).sum())} of {len(ba)} rounds",
            flush=True)
    v.close()


if __name__ == "__main__":
    main()
