#!/usr/bin/env python3
"""What the client replies cost: N executed requests -> N signed reply texts, in one process.

  (a*) the path a caller had before pbft_sign_replies, through the entry points that existed then: C | result gathered
       into one buffer on the host (the 64-byte client fields normalised, numpy), pbft_digest_blake2b512 (blocking), the
       kind-3 envelopes built on the host, pbft_sign_batch (which re-derives the key in every lane and copies R and S to
       the host), R || S merged, then one C loop over the replies (pbft_wire_encode_replies with the signatures handed
       in), which has no per-call overhead;
  (b)  pbft_sign_replies: the blocking form (results up, texts, digests and signatures down);
  (c)  pbft_sign_replies_device alone, HIP events around its three kernels.

The outputs are compared byte for byte before anything is timed.  (a*) and (b) alternate; the outer time is a host clock
around calls that end in a synchronise.  Workloads, all canonical: 2,048 replies (what every replica owes the clients of
a 2^20-vote round) with the 8-byte result "awesome!" and with 1,024-byte results.  The condition on speed: (b)'s median
is not above (a*)'s by more than (a*)'s own min-max spread.
usage: python tools/reply_probe.py [--reps 30] [--n 2048] [--out FILE.json]"""
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
    seed = np.frombuffer(hashlib.sha512(b"reply-probe").digest()[:32], np.uint8).copy()
    replica, view = 2, 1
    pub = v.set_signing_seed(seed.tobytes(), replica)
    pid = np.frombuffer(wire.peer_id_b58(pub.tobytes()), np.uint8).copy()
    n = a.n
    out = {"reps": a.reps, "replica": replica, "n": n, "workloads": {}}

    def pinned(shape, dtype=np.uint8):
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return torch.zeros(max(nbytes, 1), dtype=torch.uint8).pin_memory().numpy()[:nbytes].view(dtype).reshape(shape)

    rng = np.random.default_rng(n)
    alpha = np.array([c for c in range(0x20, 0x7F) if c not in (0x22, 0x5C)], np.uint8)  # the canonical alphabet
    workloads = {"awesome_8B": [b"awesome!"] * n,
                 "results_1024B": [alpha[rng.integers(0, len(alpha), 1024)].tobytes() for _ in range(n)]}
    for name, results in workloads.items():
        packed = wire.pack_results(results, np.arange(1, n + 1), ["127.0.0.1:%d" % (8000 + i % 100) for i in range(n)])
        res_bytes = packed[1]
        data, off, ln, ts, cl = (pinned(x.shape, x.dtype) for x in (packed[0], packed[2], packed[3], packed[4], packed[5]))
        for dst, src in zip((data, off, ln, ts, cl), (packed[0], packed[2], packed[3], packed[4], packed[5])):
            dst[...] = src
        req = (v._ctx, data.ctypes.data, res_bytes, off.ctypes.data, ln.ctypes.data, ts.ctypes.data, cl.ctypes.data)
        need = ctypes.c_size_t()
        lib.pbft_sign_replies(*req, view, n, None, 0, ctypes.byref(need), None, None, None, None)
        total = need.value
        out_a, out_b = pinned(total), pinned(total)
        dig_a, R, S, sig_a = pinned((n, 64)), pinned((n, 32)), pinned((n, 32)), pinned((n, 64))
        env = pinned((n, 85))
        idx = np.zeros(n, np.uint16)
        off_b, dig_b, sig_b, st_b = pinned(n + 1, np.int64), pinned((n, 64)), pinned((n, 64)), pinned(n)
        # (a*)'s gather buffer: C | result per reply, back to back
        g_len = (64 + ln.astype(np.int64)).astype(np.uint32)
        g_off = (np.cumsum(g_len, dtype=np.uint64) - g_len).astype(np.uint64)
        gather = pinned(int(g_len.sum()) + 16)
        lens64, offs64, goff64 = ln.astype(np.int64), off.astype(np.int64), g_off.astype(np.int64)
        uniform = int(lens64.min()) == int(lens64.max())

        def gather_digest():
            # C: everything from the first NUL on replaced by zeros
            open_ = np.logical_and.accumulate(cl != 0, axis=1)
            c = np.where(open_, cl, 0).astype(np.uint8)
            if uniform:  # one reshape: every row is C | result
                k = int(lens64[0])
                rows = gather[:n * (64 + k)].reshape(n, 64 + k)
                rows[:, :64] = c
                rows[:, 64:] = data[:n * k].reshape(n, k)
            else:
                for i in range(n):
                    g = int(goff64[i])
                    gather[g:g + 64] = c[i]
                    gather[g + 64:g + 64 + int(lens64[i])] = data[int(offs64[i]):int(offs64[i]) + int(lens64[i])]
            check(lib.pbft_digest_blake2b512(v._ctx, gather.ctypes.data, g_off.ctypes.data, g_len.ctypes.data, n,
                                             dig_a.ctypes.data))

        def envelopes_and_sign():
            env[:, :4] = np.frombuffer(b"PBFT", np.uint8)
            env[:, 4] = wire.KIND_REPLY
            env[:, 5:13] = np.full(n, view, "<u8").reshape(n, 1).view(np.uint8)
            env[:, 13:21] = ts.astype("<u8").reshape(n, 1).view(np.uint8)
            env[:, 21:] = dig_a
            check(lib.pbft_sign_batch(v._ctx, seed.ctypes.data, 1, idx.ctypes.data, env.ctypes.data, 85, 85, n,
                                      R.ctypes.data, S.ctypes.data, None))
            sig_a[:, :32] = R
            sig_a[:, 32:] = S

        def encode_c_loop(dst):
            check(lib.pbft_wire_encode_replies(n, view, ts.ctypes.data, data.ctypes.data, off.ctypes.data, ln.ctypes.data,
                                               replica, pid.ctypes.data, sig_a.ctypes.data, dst.ctypes.data, total,
                                               ctypes.byref(need), None, None))

        def leg_a_star():
            gather_digest()
            envelopes_and_sign()
            encode_c_loop(out_a)

        def leg_b():
            check(lib.pbft_sign_replies(*req, view, n, out_b.ctypes.data, total, ctypes.byref(need), off_b.ctypes.data,
                                        dig_b.ctypes.data, sig_b.ctypes.data, st_b.ctypes.data))

        d_in = [torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
                for x in (data, off, ln, ts, cl)]
        d_out = torch.zeros(total + 64, dtype=torch.uint8, device=dev)
        d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_dig, d_sig = (torch.zeros(64 * n, dtype=torch.uint8, device=dev) for _ in range(2))
        d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
        v.reply_reserve(n)
        st = torch.cuda.Stream(dev)
        p = [t.data_ptr() for t in d_in]

        def leg_c():
            v.sign_replies_device(p[0], res_bytes, p[1], p[2], p[3], p[4], view, n, d_out.data_ptr(), total,
                                  d_off.data_ptr(), d_dig.data_ptr(), d_sig.data_ptr(), d_st.data_ptr(),
                                  stream=st.cuda_stream)

        # 1. outputs first
        leg_a_star()
        leg_b()
        assert need.value == total and out_a.tobytes() == out_b.tobytes()
        assert (sig_b == sig_a).all() and (dig_b == dig_a).all() and not st_b.any()
        leg_c()
        st.synchronize()
        assert d_out.cpu().numpy()[:total].tobytes() == out_a.tobytes()
        assert int(d_off.cpu().numpy()[-1]) == total
        res = {"stream_bytes": total, "results_bytes": int(res_bytes),
               "checked": "(a*), (b) and (c) write the same bytes, digests and signatures"}

        # 2. (a*) and (b), alternating
        for _ in range(3):
            leg_a_star()
            leg_b()
        t_as, t_b = [], []
        for _ in range(a.reps):
            for leg, acc in ((leg_a_star, t_as), (leg_b, t_b)):
                t0 = time.perf_counter()
                leg()
                acc.append((time.perf_counter() - t0) * 1e3)
        res["a_star_gather_digest_sign_batch_and_c_loop_encode_ms"] = stats(t_as)
        res["b_sign_replies_ms"] = stats(t_b)
        parts = {"gather_and_pbft_digest_blake2b512": [], "envelopes_pbft_sign_batch_merge": [], "c_loop_encode": []}
        for _ in range(a.reps):  # the parts of (a*), apart
            t0 = time.perf_counter()
            gather_digest()
            t1 = time.perf_counter()
            envelopes_and_sign()
            t2 = time.perf_counter()
            encode_c_loop(out_a)
            t3 = time.perf_counter()
            parts["gather_and_pbft_digest_blake2b512"].append((t1 - t0) * 1e3)
            parts["envelopes_pbft_sign_batch_merge"].append((t2 - t1) * 1e3)
            parts["c_loop_encode"].append((t3 - t2) * 1e3)
        res["a_star_parts_ms"] = {k: stats(x) for k, x in parts.items()}
        sa, sb = res["a_star_gather_digest_sign_batch_and_c_loop_encode_ms"], res["b_sign_replies_ms"]
        res["condition_b_not_above_a_star_by_more_than_its_spread"] = {
            "b_minus_a_star_median_ms": sb["median"] - sa["median"], "a_star_spread_ms": sa["max"] - sa["min"],
            "met": bool(sb["median"] - sa["median"] <= sa["max"] - sa["min"])}

        # 3. (c), the kernels alone
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
        res["c_device_kernels_ms"] = stats(ms)
        out["workloads"][name] = res
    out["public_key"] = pub.tobytes().hex()
    out["note"] = ("(a*), (b): wall clock of blocking calls on one host thread, pinned host buffers; (c): HIP events "
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
