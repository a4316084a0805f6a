#!/usr/bin/env python3
"""What a replica's own votes cost: N envelopes -> N signed UviBytes/JSON vote frames, three ways in one process.

  (a) the per-event path as it was: pbft_sign_batch (which re-derives the key in every lane and copies R and S to the
      host), R || S merged and pbft_wire_encode_votes on the host thread, from and into pinned buffers;
  (b) pbft_sign_votes_frames: the blocking form of the GPU egress (envelopes up, frames down);
  (c) pbft_sign_votes_frames_device alone, HIP events around its three kernels, in every form of the signing kernel:
      64 or 256 lanes per workgroup (PBFT_OPT_EGRESS_BLOCK), the wave's frames staged in LDS and stored with 16-byte
      stores or every lane storing its own frame bytewise (PBFT_OPT_EGRESS_DIRECT).

The three outputs are compared byte for byte before anything is timed.  (a) and (b) alternate; the outer time is a host
clock around calls that end in a synchronise.  Sizes: 4,096 (the replies to a 2^20-vote round with 2,048 PrePrepares)
and 2^16.  The condition on speed: (b)'s median is not above (a)'s by more than (a)'s own min-max spread.
usage: python tools/egress_probe.py [--reps 30] [--sizes 4096,65536] [--out FILE.json]"""
import argparse
import ctypes
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(x):
    import numpy as np
    x = np.array(x)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max())}


def main():
    import numpy as np
    import torch
    from pbft_amd import GpuBatchVerifier
    from pbft_amd._lib import check
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sizes", default="4096,65536")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    v = GpuBatchVerifier(0)
    lib = v._lib
    seed = np.frombuffer(hashlib.sha512(b"egress-probe").digest()[:32], np.uint8).copy()
    replica, view = 7, 1
    pub = v.set_signing_seed(seed.tobytes(), replica)
    out = {"reps": a.reps, "replica": replica, "sizes": {}}

    def pinned(shape, dtype=np.uint8):
        return torch.zeros(shape, dtype=getattr(torch, np.dtype(dtype).name)).pin_memory().numpy()

    for n in [int(s) for s in a.sizes.split(",")]:
        rng = np.random.default_rng(n)
        env = pinned((n, 85))
        env[:, :4] = np.frombuffer(b"PBFT", np.uint8)
        env[:, 4] = 1 + (np.arange(n) & 1)  # a Prepare and a Commit per seq, as the events of a round come
        env[:, 5:13] = np.full(n, view, "<u8").reshape(n, 1).view(np.uint8)
        env[:, 13:21] = (1 + (np.arange(n) >> 1)).astype("<u8").reshape(n, 1).view(np.uint8)
        env[:, 21:] = rng.integers(0, 256, (n, 64), dtype=np.uint8)
        kind = env[:, 4].copy()
        vw = np.full(n, view, np.uint64)
        sq = (1 + (np.arange(n) >> 1)).astype(np.uint64)
        dig = env[:, 21:].copy()
        rep = np.full(n, replica, np.uint32)
        idx = np.zeros(n, np.uint16)
        R, S, sigs = pinned((n, 32)), pinned((n, 32)), pinned((n, 64))
        need = ctypes.c_size_t()
        lib.pbft_sign_votes_frames(v._ctx, env.ctypes.data, 85, n, None, 0, ctypes.byref(need), None, None)  # the length
        total = need.value
        out_a, out_b = pinned(total), pinned(total)
        off_b, sig_b = pinned(n + 1, np.int64), pinned((n, 64))

        def leg_a():
            check(lib.pbft_sign_batch(v._ctx, seed.ctypes.data, 1, idx.ctypes.data, env.ctypes.data, 85, 85, n,
                                      R.ctypes.data, S.ctypes.data, None))
            sigs[:, :32] = R
            sigs[:, 32:] = S
            check(lib.pbft_wire_encode_votes(n, kind.ctypes.data, vw.ctypes.data, sq.ctypes.data, dig.ctypes.data,
                                             rep.ctypes.data, sigs.ctypes.data, out_a.ctypes.data, total,
                                             ctypes.byref(need)))

        def leg_b():
            check(lib.pbft_sign_votes_frames(v._ctx, env.ctypes.data, 85, n, out_b.ctypes.data, total,
                                             ctypes.byref(need), off_b.ctypes.data, sig_b.ctypes.data))

        d_env = torch.from_numpy(env.reshape(-1).copy()).to(dev)
        d_out = torch.zeros(total + 64, dtype=torch.uint8, device=dev)
        d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_sig = torch.zeros(64 * n, dtype=torch.uint8, device=dev)
        v.egress_reserve(n)
        st = torch.cuda.Stream(dev)

        def leg_c():
            v.sign_votes_frames_device(d_env.data_ptr(), n, d_out.data_ptr(), total, d_off.data_ptr(),
                                       d_sig.data_ptr(), stream=st.cuda_stream)

        # 1. outputs first
        leg_a()
        leg_b()
        assert need.value == total and out_a.tobytes() == out_b.tobytes() and (sig_b == sigs).all()
        forms = [(64, 0), (256, 0), (64, 1), (256, 1)]
        for block, direct in forms:
            v.set_option(v.OPT_EGRESS_BLOCK, block)
            v.set_option(v.OPT_EGRESS_DIRECT, direct)
            d_out.zero_()
            leg_c()
            st.synchronize()
            assert d_out.cpu().numpy()[:total].tobytes() == out_a.tobytes(), (block, direct)
            assert int(d_off.cpu().numpy()[-1]) == total
        v.set_option(v.OPT_EGRESS_BLOCK, 0)
        v.set_option(v.OPT_EGRESS_DIRECT, 0)
        res = {"stream_bytes": total, "checked": "(a), (b) and every form of (c) write the same bytes"}

        # 2. (a) and (b), alternating
        for _ in range(3):
            leg_a()
            leg_b()
        ta, tb = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            leg_a()
            ta.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            leg_b()
            tb.append((time.perf_counter() - t0) * 1e3)
        res["a_sign_batch_and_host_encode_ms"] = stats(ta)
        res["b_sign_votes_frames_ms"] = stats(tb)
        # the parts of (a), apart
        ts, te = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            check(lib.pbft_sign_batch(v._ctx, seed.ctypes.data, 1, idx.ctypes.data, env.ctypes.data, 85, 85, n,
                                      R.ctypes.data, S.ctypes.data, None))
            t1 = time.perf_counter()
            sigs[:, :32] = R
            sigs[:, 32:] = S
            check(lib.pbft_wire_encode_votes(n, kind.ctypes.data, vw.ctypes.data, sq.ctypes.data, dig.ctypes.data,
                                             rep.ctypes.data, sigs.ctypes.data, out_a.ctypes.data, total,
                                             ctypes.byref(need)))
            ts.append((t1 - t0) * 1e3)
            te.append((time.perf_counter() - t1) * 1e3)
        res["a_parts_ms"] = {"pbft_sign_batch": stats(ts), "merge_and_pbft_wire_encode_votes": stats(te)}
        sa, sb = res["a_sign_batch_and_host_encode_ms"], res["b_sign_votes_frames_ms"]
        res["condition_b_not_above_a_by_more_than_a_spread"] = {
            "b_minus_a_median_ms": sb["median"] - sa["median"], "a_spread_ms": sa["max"] - sa["min"],
            "met": bool(sb["median"] - sa["median"] <= sa["max"] - sa["min"])}

        # 3. (c), the kernels alone, every form
        res["c_device_kernels_ms"] = {}
        for block, direct in forms:
            v.set_option(v.OPT_EGRESS_BLOCK, block)
            v.set_option(v.OPT_EGRESS_DIRECT, direct)
            ms = []
            for r in range(a.reps + 3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                with torch.cuda.stream(st):
                    e0.record(st)
                    leg_c()
                    e1.record(st)
                torch.cuda.synchronize()
                if r >= 3:
                    ms.append(e0.elapsed_time(e1))
            res["c_device_kernels_ms"]["block%d_%s" % (block, "direct" if direct else "staged")] = stats(ms)
        v.set_option(v.OPT_EGRESS_BLOCK, 0)
        v.set_option(v.OPT_EGRESS_DIRECT, 0)
        out["sizes"][str(n)] = res
    out["public_key"] = pub.tobytes().hex()
    out["note"] = ("(a), (b): wall clock of blocking calls on one host thread, pinned host buffers; (c): HIP events "
                   "around the three kernels of one device call")
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    v.close()


if __name__ == "__main__":
    main()
