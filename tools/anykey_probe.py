#!/usr/bin/env python3
"""Cost of verifying under uninstalled keys next to the table path: pbft_verify_batch_keys_device (every signature under
its own key, the key carried inline) and pbft_verify_batch_device (256 installed keys) at the same N on the same context,
HIP events around each launch, interleaved, medians.  85-byte envelopes, 0.1 % of the signatures corrupted; every case's
bits are checked first.  Then, once, what a caller without this path has to do for 2,048 signatures under 2,048 new
keys: pbft_verify_set_keys with all of them followed by pbft_verify_batch, on a fresh context, host wall time; next to it
the blocking host form pbft_verify_batch_keys on the same signatures.  Kernel durations come from a separate
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/anykey_probe.py --sizes <one> --no-alt` run.
usage: python tools/anykey_probe.py [--reps R] [--sizes 2048,65536,1048576] [--no-alt] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (2048, 65536, 1 << 20)
ALT_N = 2048


def main():
    import numpy as np
    import torch
    import bench
    from pbft_amd import GpuBatchVerifier, SigBatch, bitmap_to_bool
    from pbft_amd._lib import LIB_PATH
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES))
    ap.add_argument("--no-alt", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",") if s]
    n_max = max(sizes + [ALT_N])
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    v = GpuBatchVerifier(0)
    v.set_option(v.OPT_KERNEL_TIMING, 0)
    rng = np.random.default_rng(bench.SEED)
    msg = np.zeros((n_max, bench.ENVELOPE), np.uint8)
    msg[:, :4] = np.frombuffer(b"PBFT", np.uint8)
    msg[:, 4] = 1 + (np.arange(n_max) & 1)
    msg[:, 5:] = rng.integers(0, 256, (n_max, bench.ENVELOPE - 5), dtype=np.uint8)
    # distinct keys: the signer takes a 16-bit seed index, so 65,536 seeds at a time
    seeds = rng.integers(0, 256, (n_max, 32), dtype=np.uint8)
    R1, S1, A1 = (np.zeros((n_max, 32), np.uint8) for _ in range(3))
    for lo in range(0, n_max, 65536):
        hi = min(lo + 65536, n_max)
        r, s, pub = v.sign(seeds[lo:hi], np.arange(hi - lo, dtype=np.uint16), msg[lo:hi], bench.ENVELOPE)
        R1[lo:hi], S1[lo:hi], A1[lo:hi] = r, s, pub
    assert len(np.unique(A1[:65536], axis=0)) == min(n_max, 65536)
    S1, bad1 = bench.corrupt(S1, bench.ADV_FRAC, bench.SEED)
    # the table path's batch: the same envelopes under 256 installed keys
    n_rep = bench.N_REPLICAS
    kidx = (np.arange(n_max) % n_rep).astype(np.uint16)
    R2, S2, pub2 = v.sign(bench.key_seeds(n_rep), kidx, msg, bench.ENVELOPE)
    S2, bad2 = bench.corrupt(S2, bench.ADV_FRAC, bench.SEED + 1)
    exp1, exp2 = np.ones(n_max, bool), np.ones(n_max, bool)
    exp1[bad1] = False
    exp2[bad2] = False
    out = {"reps": a.reps, "lib": os.path.basename(LIB_PATH), "envelope_bytes": bench.ENVELOPE,
           "note": "HIP events on the launch stream around one device-form call (sum kernel + finish, or comb + finish); "
                   "keys: every signature under its own key, inline; table: 256 installed keys"}
    mp = np.zeros(n_max * bench.ENVELOPE + 64, np.uint8)
    mp[: n_max * bench.ENVELOPE] = msg.reshape(-1)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    d = {"M": up(mp), "R1": up(R1), "S1": up(S1), "A1": up(A1), "R2": up(R2), "S2": up(S2),
         "K2": up(kidx.view(np.int16)), "B": torch.zeros((n_max + 63) // 64, dtype=torch.int64, device=dev)}
    assert v.set_keys(pub2).all()
    v.reserve(max(sizes))
    st = torch.cuda.Stream(dev)
    E = bench.ENVELOPE

    def keys_form(n):
        v.verify_keys_device(d["R1"].data_ptr(), d["S1"].data_ptr(), d["A1"].data_ptr(), d["M"].data_ptr(), E, E, n,
                             d["B"].data_ptr(), st.cuda_stream)

    def table_form(n):
        v.verify_device(d["R2"].data_ptr(), d["S2"].data_ptr(), d["K2"].data_ptr(), d["M"].data_ptr(), E, E, n,
                        d["B"].data_ptr(), st.cuda_stream)
    forms = (("keys", keys_form, exp1), ("table", table_form, exp2))
    for n in sizes:  # warm, and check
        for name, f, exp in forms:
            for _ in range(2):
                f(n)
            torch.cuda.synchronize()
            got = bitmap_to_bool(d["B"].cpu().numpy().view(np.uint64)[: (n + 63) // 64], n)
            assert (got == exp[:n]).all(), (name, n)
    ms = {(name, n): [] for name, _, _ in forms for n in sizes}
    for rep in range(a.reps):
        for n in sizes:  # interleaved
            for name, f, _ in forms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(st)
                f(n)
                e1.record(st)
                torch.cuda.synchronize()
                ms[(name, n)].append(e0.elapsed_time(e1))
    for n in sizes:
        k, t = np.array(ms[("keys", n)]), np.array(ms[("table", n)])
        out[str(n)] = {"keys_ms_median": float(np.median(k)), "keys_ms_min": float(k.min()), "keys_ms_max": float(k.max()),
                       "keys_verifies_per_s": float(n / np.median(k) * 1e3),
                       "table_ms_median": float(np.median(t)), "table_ms_min": float(t.min()),
                       "table_ms_max": float(t.max()), "table_verifies_per_s": float(n / np.median(t) * 1e3),
                       "keys_over_table": float(np.median(k) / np.median(t))}
    v.close()
    if not a.no_alt:
        # the caller's alternative before this path, once: install the 2,048 keys, then verify under them
        v2 = GpuBatchVerifier(0)
        n = ALT_N
        idx = np.arange(n, dtype=np.uint16)
        v2.verify_keys(R1[:64], S1[:64], A1[:64], msg[:64], E)  # (first launch: code objects loaded)
        t0 = time.perf_counter()
        bm = v2.verify_keys(R1[:n], S1[:n], A1[:n], msg[:n], E)
        t1 = time.perf_counter()
        assert (bitmap_to_bool(bm, n) == exp1[:n]).all()
        t2 = time.perf_counter()
        ok = v2.set_keys(A1[:n])
        t3 = time.perf_counter()
        bm = v2.verify(SigBatch(R1[:n], S1[:n], idx, msg[:n], E))
        t4 = time.perf_counter()
        assert ok.all() and (bitmap_to_bool(bm, n) == exp1[:n]).all()
        out["alternative_2048"] = {"set_keys_ms": (t3 - t2) * 1e3, "verify_batch_ms": (t4 - t3) * 1e3,
                                   "set_keys_plus_verify_ms": (t4 - t2) * 1e3,
                                   "verify_batch_keys_host_ms": (t1 - t0) * 1e3,
                                   "ratio": (t4 - t2) / (t1 - t0), "key_stats": v2.key_stats(),
                                   "note": "host wall time, one run each, blocking host forms, PCIe copies included"}
        v2.close()
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
