#!/usr/bin/env python3
"""Cost of the vote tally next to the verify it follows: device-resident config-#4 rows (n = 256 signers, 4,096
envelopes), pbft_verify_votes_device + pbft_tally_device on one stream, at N = 2^20 and at the 131,072-row shard,
each with the rows in the replica's order (an envelope's votes contiguous) and fully permuted.  Per case: HIP events
around the verify and around the tally (zero + tally + count kernels), interleaved over the cases, medians;
every case's sets and counts are checked against tally_reference first.  Kernel durations come from a separate
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/tally_probe.py --cases <one case>` run.
usage: python tools/tally_probe.py [--reps R] [--cases sorted_1048576,permuted_131072,...] [--out FILE.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("sorted_1048576", "permuted_1048576", "sorted_131072", "permuted_131072")


def main():
    import numpy as np
    import torch
    import bench
    from pbft_amd import GpuBatchVerifier, bitmap_to_bool, tally_reference
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    cases = [c for c in a.cases.split(",") if c]
    assert all(c in CASES for c in cases), cases
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    n_sig, n_env = bench.N_REPLICAS, 2 * bench.SEQS
    seeds = bench.key_seeds(n_sig)
    msg, key_idx = bench.envelopes(1, bench.SEQS, n_sig)
    v = GpuBatchVerifier(0)
    v.set_option(v.OPT_KERNEL_TIMING, 0)
    R, S_good, pub = v.sign(seeds, key_idx, msg, bench.ENVELOPE)
    S, bad = bench.corrupt(S_good, bench.ADV_FRAC, bench.SEED)
    n_all = len(msg)
    expect = np.ones(n_all, bool)
    expect[bad] = False
    assert v.set_keys(pub).all()
    env = msg[::n_sig].copy()                              # round order: envelope e = rows [256 e, 256 e + 256)
    env_idx = (np.arange(n_all) // n_sig).astype(np.uint32)
    envp = np.zeros(n_env * bench.ENVELOPE + 64, np.uint8)
    envp[: n_env * bench.ENVELOPE] = env.reshape(-1)
    dE = torch.from_numpy(envp).to(dev)
    perm = np.random.default_rng(bench.SEED).permutation(n_all)
    st = torch.cuda.Stream(dev)
    W = (n_sig + 63) // 64
    run = {}
    for c in cases:
        order, n = c.split("_")
        n = int(n)
        p = (perm if order == "permuted" else np.arange(n_all))[:n]
        d = {"R": torch.from_numpy(R[p]).to(dev), "S": torch.from_numpy(S[p]).to(dev),
             "K": torch.from_numpy(key_idx[p].view(np.int16)).to(dev),
             "I": torch.from_numpy(env_idx[p].view(np.int32)).to(dev),
             "B": torch.zeros((n + 63) // 64, dtype=torch.int64, device=dev),
             "sets": torch.zeros(n_env * W, dtype=torch.int64, device=dev),
             "cnt": torch.zeros(n_env, dtype=torch.int32, device=dev)}
        v.reserve(n)

        def verify(d=d, n=n):
            v.verify_votes_device(d["R"].data_ptr(), d["S"].data_ptr(), d["K"].data_ptr(), d["I"].data_ptr(),
                                  dE.data_ptr(), n_env, n, d["B"].data_ptr(), st.cuda_stream)

        def tally(d=d, n=n):
            v.tally_device(d["B"].data_ptr(), d["K"].data_ptr(), d["I"].data_ptr(), n, n_env, n_sig,
                           d["sets"].data_ptr(), d["cnt"].data_ptr(), st.cuda_stream)
        for _ in range(3):  # warm, and check
            verify()
            tally()
        torch.cuda.synchronize()
        assert (bitmap_to_bool(d["B"].cpu().numpy().view(np.uint64), n) == expect[p]).all(), c
        exp_s, exp_c = tally_reference(expect[p], key_idx[p], env_idx[p], n_env, n_sig)
        assert (d["sets"].cpu().numpy().view(np.uint64).reshape(n_env, W) == exp_s).all(), c
        assert (d["cnt"].cpu().numpy().view(np.uint32) == exp_c).all(), c
        run[c] = (verify, tally, d, {"verify_ms": [], "tally_ms": []})
    for rep in range(a.reps + 1):
        for c in cases:  # interleaved
            verify, tally, d, res = run[c]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            torch.cuda.synchronize()
            ev[0].record(st)
            verify()
            ev[1].record(st)
            tally()
            ev[2].record(st)
            torch.cuda.synchronize()
            if rep:
                res["verify_ms"].append(ev[0].elapsed_time(ev[1]))
                res["tally_ms"].append(ev[1].elapsed_time(ev[2]))
    out = {"reps": a.reps, "n_signers": n_sig, "n_env": n_env,
           "note": "HIP events on the launch stream; tally = tally_zero_kernel + tally_kernel + tally_count_kernel"}
    for c in cases:
        res = run[c][3]
        vm, tm = np.array(res["verify_ms"]), np.array(res["tally_ms"])
        out[c] = {"verify_ms_median": float(np.median(vm)), "tally_ms_median": float(np.median(tm)),
                  "tally_ms_min": float(tm.min()), "tally_ms_max": float(tm.max()),
                  "tally_share_of_verify": float(np.median(tm) / np.median(vm))}
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    v.close()


if __name__ == "__main__":
    main()
