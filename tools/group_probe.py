#!/usr/bin/env python3
"""Cost of the envelope grouping (pbft_group_envelopes_device) at 2^20 records of the config-#4 round (n = 256
signers, 4,096 envelopes), read in place from 160-byte wire records.
--part device: HIP events around the grouping's five kernels, around pbft_verify_records_device of the same records
  (comb + finish) and around a plain device-to-device copy that moves the grouping's algorithmic bytes (85 of each
  record read + 4 bytes per row written; the copy reads half of that and writes half), interleaved over the cases,
  medians.  Cases: replica (an envelope's 256 votes contiguous), permuted, and the two adversarial shapes: distinct
  (every row its own envelope, env_cap = N) and equal (one envelope).  The adversarial cases carry no valid
  signatures and are timed for the grouping alone.
--part host: wall clock of the blocking pbft_verify_frames_tally next to pbft_verify_frames on the same stream of
  2^20 canonical frames in pinned host memory (the added cost), and the bytes each returns per vote.
Every output is checked against group_reference / tally_reference / the expected bits before anything is timed.
usage: python tools/group_probe.py [--part device|host|all] [--reps R] [--log2n 20] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("replica", "permuted", "distinct", "equal")


def pinned(a):
    import torch
    return torch.from_numpy(a).pin_memory().numpy()


def main():
    import numpy as np
    import torch
    import bench
    from pbft_amd import FrameHead, GpuBatchVerifier, bitmap_to_bool, group_reference, tally_reference, wire
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("device", "host", "all"), default="all")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    n_sig = bench.N_REPLICAS
    n = 1 << a.log2n
    n_env = n // n_sig
    seeds = bench.key_seeds(n_sig)
    msg, key_idx = bench.envelopes(1, n // (2 * n_sig), n_sig)
    v = GpuBatchVerifier(0)
    R, S_good, pub = v.sign(seeds, key_idx, msg, bench.ENVELOPE)
    S, bad = bench.corrupt(S_good, bench.ADV_FRAC, bench.SEED)
    expect = np.ones(n, bool)
    expect[bad] = False
    assert v.set_keys(pub).all()
    words, W = (n + 63) // 64, (n_sig + 63) // 64
    out = {"n": n, "n_signers": n_sig, "n_env": n_env, "reps": a.reps}
    lib = v._lib
    if a.part in ("device", "all"):
        records = wire.records_pack(R, S, key_idx, msg)
        perm = np.random.default_rng(bench.SEED).permutation(n)
        algo_bytes = (85 + 4) * n
        src = torch.zeros(algo_bytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.zeros(algo_bytes // 2, dtype=torch.uint8, device=dev)
        v.reserve(n)
        v.group_reserve(n)
        st = torch.cuda.Stream(dev)
        run = {}
        for c in CASES:
            rec, signed, cap = records, True, n_env
            if c == "permuted":
                rec = records[perm]
            elif c == "distinct":
                rec, signed, cap = records.copy(), False, n
                rec[:, 64 + 13:64 + 21] = np.arange(n, dtype="<u8").view(np.uint8).reshape(n, 8)
            elif c == "equal":
                rec, signed = records.copy(), False
                rec[:, 64:149] = records[0, 64:149]
            d = {"rec": torch.from_numpy(rec).to(dev), "idx": torch.zeros(n, dtype=torch.int32, device=dev),
                 "env": torch.zeros(cap * 85 + 64, dtype=torch.uint8, device=dev),
                 "n_env": torch.zeros(2, dtype=torch.int32, device=dev),
                 "B": torch.zeros(words, dtype=torch.int64, device=dev)}

            def group(d=d, cap=cap):
                p = d["rec"].data_ptr()
                v.group_envelopes_device(p + 64, n, cap, d["idx"].data_ptr(), d["env"].data_ptr(),
                                         d["n_env"].data_ptr(), msg_stride=160, d_key_idx=p + 150, key_stride=160,
                                         stream=st.cuda_stream)

            def verify(d=d):
                assert lib.pbft_verify_records_device(v._ctx, d["rec"].data_ptr(), n, d["B"].data_ptr(),
                                                      st.cuda_stream) == 0
            for _ in range(2):  # warm, and check
                group()
                if signed:
                    verify()
            torch.cuda.synchronize()
            e_idx, e_env, e_n = group_reference(rec[:, 64:149], None, cap)
            assert (d["idx"].cpu().numpy().view(np.uint32) == e_idx).all(), c
            assert (d["env"].cpu().numpy()[:cap * 85].reshape(cap, 85) == e_env).all(), c
            assert (d["n_env"].cpu().numpy().view(np.uint32) == e_n).all(), c
            if signed:
                order = perm if c == "permuted" else np.arange(n)
                assert (bitmap_to_bool(d["B"].cpu().numpy().view(np.uint64), n) == expect[order]).all(), c
            run[c] = (group, verify, signed, {"group_ms": [], "verify_ms": [], "copy_ms": []}, int(e_n[0]))
        for rep in range(a.reps + 1):
            for c in CASES:  # interleaved
                group, verify, signed, res, _ = run[c]
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                torch.cuda.synchronize()
                with torch.cuda.stream(st):
                    ev[0].record(st)
                    group()
                    ev[1].record(st)
                    if signed:
                        verify()
                    ev[2].record(st)
                    dst.copy_(src)
                    ev[3].record(st)
                torch.cuda.synchronize()
                if rep:
                    for k, name in enumerate(("group_ms", "verify_ms", "copy_ms")):
                        res[name].append(ev[k].elapsed_time(ev[k + 1]))
        dev_out = {"algorithmic_bytes": algo_bytes,
                   "note": "HIP events on the launch stream; group = fill + insert + mark + scan + assign kernels; "
                           "verify = comb + finish of the same records; floor = a D2D copy moving algorithmic_bytes"}
        for c in CASES:
            _, _, signed, res, found = run[c]
            g, f = np.array(res["group_ms"]), float(np.median(res["copy_ms"]))
            r = {"envelopes_found": found, "group_ms_median": float(np.median(g)), "group_ms_min": float(g.min()),
                 "group_ms_max": float(g.max()), "floor_ms": f, "group_over_floor": float(np.median(g)) / f}
            if signed:
                vm = float(np.median(res["verify_ms"]))
                r.update({"verify_ms_median": vm, "group_share_of_verify": float(np.median(g)) / vm})
            dev_out[c] = r
        dev_out["equal_over_replica"] = dev_out["equal"]["group_ms_median"] / dev_out["replica"]["group_ms_median"]
        dev_out["distinct_over_replica"] = (dev_out["distinct"]["group_ms_median"] /
                                            dev_out["replica"]["group_ms_median"])
        out["device"] = dev_out
    if a.part in ("host", "all"):
        kind = msg[:, 4].copy()
        view = msg[:, 5:13].copy().view(np.uint64).reshape(n)
        seq = msg[:, 13:21].copy().view(np.uint64).reshape(n)
        stream = wire.encode_votes(kind, view, seq, msg[:, 21:], key_idx.astype(np.uint32),
                                   np.concatenate([R, S], axis=1))
        off, flen, used = wire.frame_index(stream)
        assert len(off) == n and used == len(stream)
        h_stream, h_off, h_len = pinned(stream), pinned(off), pinned(flen)
        h_bm, h_heads = pinned(np.zeros(words, np.uint64)), pinned(np.zeros(n, FrameHead).view(np.uint8))
        h_rec = pinned(np.zeros((n, 160), np.uint8))
        h_env, h_n = pinned(np.zeros((n_env, 85), np.uint8)), pinned(np.zeros(2, np.uint32))
        h_sets, h_cnt = pinned(np.zeros((n_env, W), np.uint64)), pinned(np.zeros(n_env, np.uint32))
        h_idx = pinned(np.zeros(n, np.uint32))

        def frames(rec=None):
            rc = lib.pbft_verify_frames(v._ctx, h_stream.ctypes.data, len(stream), h_off.ctypes.data, h_len.ctypes.data,
                                        None, n_sig, n, h_bm.ctypes.data, h_heads.ctypes.data, rec)
            assert rc == 0, lib.pbft_last_error()

        def frames_records():
            frames(h_rec.ctypes.data)

        def frames_tally(idx=None):
            rc = lib.pbft_verify_frames_tally(v._ctx, h_stream.ctypes.data, len(stream), h_off.ctypes.data,
                                              h_len.ctypes.data, None, n_sig, n, n_env, h_bm.ctypes.data,
                                              h_heads.ctypes.data, idx, h_env.ctypes.data, h_n.ctypes.data,
                                              h_sets.ctypes.data, h_cnt.ctypes.data)
            assert rc == 0, lib.pbft_last_error()

        def frames_tally_idx():
            frames_tally(h_idx.ctypes.data)
        paths = (("verify_frames", frames), ("verify_frames_with_records", frames_records),
                 ("verify_frames_tally", frames_tally), ("verify_frames_tally_with_env_idx", frames_tally_idx))
        for name, fn in paths:  # warm (the staging grows), and check
            for _ in range(2):
                fn()
            assert (bitmap_to_bool(h_bm.copy(), n) == expect).all(), name
        e_idx, e_env, e_n = group_reference(msg, None, n_env)
        e_sets, e_cnt = tally_reference(expect, key_idx, e_idx, n_env, n_sig)
        assert (h_idx == e_idx).all() and (h_env == e_env).all() and (h_n == e_n).all()
        assert (h_sets == e_sets).all() and (h_cnt == e_cnt).all()
        t = {name: [] for name, _ in paths}
        for rep in range(a.reps):
            for name, fn in paths:  # interleaved
                t0 = time.perf_counter()
                fn()
                t[name].append(time.perf_counter() - t0)
        per_env = n_env * (85 + 8 * W + 4) + 8
        back = {"verify_frames": 24 + 1 / 8, "verify_frames_with_records": 24 + 1 / 8 + 160,
                "verify_frames_tally": 24 + 1 / 8 + per_env / n,
                "verify_frames_tally_with_env_idx": 24 + 1 / 8 + 4 + per_env / n}
        host = {"stream_bytes": int(len(stream)),
                "note": "wall clock of blocking calls on one host thread; inputs and outputs in pinned host memory"}
        for name, _ in paths:
            s = float(np.median(t[name]))
            host[name] = {"ms_median": s * 1e3, "ms_min": float(min(t[name])) * 1e3, "votes_per_s": n / s,
                          "bytes_back_per_vote": back[name]}
        host["added_ms"] = host["verify_frames_tally"]["ms_median"] - host["verify_frames"]["ms_median"]
        host["added_share"] = host["added_ms"] / host["verify_frames"]["ms_median"]
        out["host"] = host
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    v.close()


if __name__ == "__main__":
    main()
