#!/usr/bin/env python3
"""What the primary's PrePrepares cost: N client requests -> N signed UviBytes/JSON PrePrepare frames, in one process.

  (a) the path a caller had before pbft_sign_preprepares_frames: pbft_digest_blake2b512 (blocking), the envelopes built
      on the host, pbft_sign_batch (which re-derives the key in every lane and copies R and S to the host), R || S
      merged, then one frame per request on the host thread.  Two encoders are timed: (a) pbft_wire_encode_frame per
      request, called through ctypes from a loop (the call the issue names; the loop's own cost is part of it), and
      (a*) the same frames from one C loop (pbft_wire_encode_preprepares with the digests and signatures handed in),
      which has no per-call overhead and is the faster of the two: the condition is evaluated against (a*);
  (b) pbft_sign_preprepares_frames: the blocking form (requests up, frames, digests and signatures down);
  (c) pbft_sign_preprepares_frames_device alone, HIP events around its three kernels, for every width of the frame
      copy (PBFT_OPT_PROPOSE_WIDTH 1, 4, 16).

The outputs are compared byte for byte before anything is timed.  (a*), (a) and (b) alternate; the outer time is a host
clock around calls that end in a synchronise.  Workloads, all canonical: 2,048 requests (the PrePrepares of a 2^20-vote
round) with the 13-byte "testOperation" and with 1,024-byte operations.  The condition on speed: (b)'s median is not
above (a*)'s by more than (a*)'s own min-max spread.
usage: python tools/propose_probe.py [--reps 30] [--n 2048] [--out FILE.json]"""
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
    from pbft_amd import GpuBatchVerifier, wire
    from pbft_amd._lib import check
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    v = GpuBatchVerifier(0)
    lib = v._lib
    seed = np.frombuffer(hashlib.sha512(b"propose-probe").digest()[:32], np.uint8).copy()
    replica, view, first = 1, 1, 1
    pub = v.set_signing_seed(seed.tobytes(), replica)
    n = a.n
    out = {"reps": a.reps, "replica": replica, "n": n, "workloads": {}}

    def pinned(shape, dtype=np.uint8):
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return torch.zeros(max(nbytes, 1), dtype=torch.uint8).pin_memory().numpy()[:nbytes].view(dtype).reshape(shape)

    rng = np.random.default_rng(n)
    P_ALPHA = np.array([c for c in range(0x20, 0x7F) if c not in (0x22, 0x5C)], np.uint8)  # the canonical alphabet
    workloads = {"testOperation_13B": [b"testOperation"] * n,
                 "operations_1024B": [P_ALPHA[rng.integers(0, len(P_ALPHA), 1024)].tobytes() for _ in range(n)]}
    for name, ops in workloads.items():
        packed = wire.pack_requests(ops, np.arange(1, n + 1), ["127.0.0.1:8080"] * n)
        ops_bytes = packed[1]
        data, off, ln, ts, cl = (pinned(x.shape, x.dtype) for x in (packed[0], packed[2], packed[3], packed[4], packed[5]))
        for dst, src in zip((data, off, ln, ts, cl), (packed[0], packed[2], packed[3], packed[4], packed[5])):
            dst[...] = src
        req = (v._ctx, data.ctypes.data, ops_bytes, off.ctypes.data, ln.ctypes.data, ts.ctypes.data, cl.ctypes.data)
        need = ctypes.c_size_t()
        lib.pbft_sign_preprepares_frames(*req, view, first, n, None, 0, ctypes.byref(need), None, None, None, None)
        total = need.value
        out_a, out_a2, out_b = pinned(total), pinned(total), pinned(total)
        dig_a, R, S, sig_a = pinned((n, 64)), pinned((n, 32)), pinned((n, 32)), pinned((n, 64))
        env = pinned((n, 85))
        idx = np.zeros(n, np.uint16)
        off_b, dig_b, sig_b, st_b = pinned(n + 1, np.int64), pinned((n, 64)), pinned((n, 64)), pinned(n)
        seqs = (first + np.arange(n)).astype("<u8")

        def digest_and_sign():
            check(lib.pbft_digest_blake2b512(v._ctx, data.ctypes.data, off.ctypes.data, ln.ctypes.data, n,
                                             dig_a.ctypes.data))
            env[:, :4] = np.frombuffer(b"PBFT", np.uint8)
            env[:, 4] = 0
            env[:, 5:13] = np.full(n, view, "<u8").reshape(n, 1).view(np.uint8)
            env[:, 13:21] = seqs.reshape(n, 1).view(np.uint8)
            env[:, 21:] = dig_a
            check(lib.pbft_sign_batch(v._ctx, seed.ctypes.data, 1, idx.ctypes.data, env.ctypes.data, 85, 85, n,
                                      R.ctypes.data, S.ctypes.data, None))
            sig_a[:, :32] = R
            sig_a[:, 32:] = S

        def encode_c_loop(dst):
            check(lib.pbft_wire_encode_preprepares(n, view, first, *req[1:2], *req[3:], replica, dig_a.ctypes.data,
                                                   sig_a.ctypes.data, dst.ctypes.data, total, ctypes.byref(need), None,
                                                   None))

        msg = wire._Msg()
        msg.kind, msg.view, msg.digest_ok, msg.has_sig, msg.replica = wire.PREPREPARE, view, 1, 1, replica
        msg.client = b"127.0.0.1:8080"
        flen = ctypes.c_size_t()

        def encode_per_request(dst):
            at, base = 0, data.ctypes.data
            for i in range(n):
                msg.seq = first + i
                ctypes.memmove(msg.digest, dig_a[i].ctypes.data, 64)
                ctypes.memmove(msg.sig, sig_a[i].ctypes.data, 64)
                msg.operation, msg.operation_len, msg.timestamp = base + int(off[i]), int(ln[i]), int(ts[i])
                check(lib.pbft_wire_encode_frame(ctypes.byref(msg), dst.ctypes.data + at, total - at, ctypes.byref(flen)))
                at += flen.value
            assert at == total

        def leg_a_star():
            digest_and_sign()
            encode_c_loop(out_a)

        def leg_a():
            digest_and_sign()
            encode_per_request(out_a2)

        def leg_b():
            check(lib.pbft_sign_preprepares_frames(*req, view, first, n, out_b.ctypes.data, total, ctypes.byref(need),
                                                   off_b.ctypes.data, dig_b.ctypes.data, sig_b.ctypes.data,
                                                   st_b.ctypes.data))

        d_in = [torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
                for x in (data, off, ln, ts, cl)]
        d_out = torch.zeros(total + 64, dtype=torch.uint8, device=dev)
        d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_dig, d_sig = (torch.zeros(64 * n, dtype=torch.uint8, device=dev) for _ in range(2))
        d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
        v.propose_reserve(n)
        st = torch.cuda.Stream(dev)
        p = [t.data_ptr() for t in d_in]

        def leg_c():
            v.sign_preprepares_frames_device(p[0], ops_bytes, p[1], p[2], p[3], p[4], view, first, n, d_out.data_ptr(),
                                             total, d_off.data_ptr(), d_dig.data_ptr(), d_sig.data_ptr(),
                                             d_st.data_ptr(), stream=st.cuda_stream)

        # 1. outputs first
        leg_a_star()
        leg_a()
        leg_b()
        assert need.value == total and out_a.tobytes() == out_b.tobytes() == out_a2.tobytes()
        assert (sig_b == sig_a).all() and (dig_b == dig_a).all() and not st_b.any()
        widths = [1, 4, 16]
        for w in widths:
            v.set_option(v.OPT_PROPOSE_WIDTH, w)
            d_out.zero_()
            leg_c()
            st.synchronize()
            assert d_out.cpu().numpy()[:total].tobytes() == out_a.tobytes(), w
            assert int(d_off.cpu().numpy()[-1]) == total
        v.set_option(v.OPT_PROPOSE_WIDTH, 0)
        res = {"stream_bytes": total, "ops_bytes": int(ops_bytes),
               "checked": "(a*), (a), (b) and every width of (c) write the same bytes"}

        # 2. (a*), (a) and (b), alternating
        for _ in range(3):
            leg_a_star()
            leg_a()
            leg_b()
        t_as, t_a, t_b = [], [], []
        for _ in range(a.reps):
            for leg, acc in ((leg_a_star, t_as), (leg_a, t_a), (leg_b, t_b)):
                t0 = time.perf_counter()
                leg()
                acc.append((time.perf_counter() - t0) * 1e3)
        res["a_star_digest_sign_batch_and_c_loop_encode_ms"] = stats(t_as)
        res["a_digest_sign_batch_and_encode_frame_per_request_ms"] = stats(t_a)
        res["b_sign_preprepares_frames_ms"] = stats(t_b)
        # the parts of (a), apart
        parts = {"pbft_digest_blake2b512": [], "envelopes_pbft_sign_batch_merge": [], "c_loop_encode": [],
                 "encode_frame_per_request": []}
        for _ in range(a.reps):
            t0 = time.perf_counter()
            check(lib.pbft_digest_blake2b512(v._ctx, data.ctypes.data, off.ctypes.data, ln.ctypes.data, n,
                                             dig_a.ctypes.data))
            t1 = time.perf_counter()
            digest_and_sign()
            t2 = time.perf_counter()
            encode_c_loop(out_a)
            t3 = time.perf_counter()
            encode_per_request(out_a2)
            t4 = time.perf_counter()
            parts["pbft_digest_blake2b512"].append((t1 - t0) * 1e3)
            parts["envelopes_pbft_sign_batch_merge"].append((t2 - t1 - (t1 - t0)) * 1e3)
            parts["c_loop_encode"].append((t3 - t2) * 1e3)
            parts["encode_frame_per_request"].append((t4 - t3) * 1e3)
        res["a_parts_ms"] = {k: stats(x) for k, x in parts.items()}
        sa, sb = res["a_star_digest_sign_batch_and_c_loop_encode_ms"], res["b_sign_preprepares_frames_ms"]
        res["condition_b_not_above_a_star_by_more_than_its_spread"] = {
            "b_minus_a_star_median_ms": sb["median"] - sa["median"], "a_star_spread_ms": sa["max"] - sa["min"],
            "met": bool(sb["median"] - sa["median"] <= sa["max"] - sa["min"])}

        # 3. (c), the kernels alone, every width
        res["c_device_kernels_ms"] = {}
        for w in widths:
            v.set_option(v.OPT_PROPOSE_WIDTH, w)
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
            res["c_device_kernels_ms"]["width%d" % w] = stats(ms)
        v.set_option(v.OPT_PROPOSE_WIDTH, 0)
        out["workloads"][name] = res
    out["public_key"] = pub.tobytes().hex()
    out["note"] = ("(a*), (a), (b): wall clock of blocking calls on one host thread, pinned host buffers; (c): HIP events "
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
