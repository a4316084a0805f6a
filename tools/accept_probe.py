#!/usr/bin/env python3
"""What the client's side costs: N signed replies (requests x 4 replicas) -> which requests are decided, in one process.

  (a*) the client's path through the entry points that existed before pbft_accept_replies: one C loop of
       pbft_wire_decode_reply with the signer's claim checked against a PeerId table (tools/accept/accept_driver.cpp),
       pbft_reply_digests, one C loop of pbft_reply_envelope, pbft_records_pack, the records uploaded,
       pbft_verify_records_device + pbft_group_envelopes_device + pbft_tally_device on them (pbft_verify_records keeps
       its upload to itself, so its device form runs on the one upload the grouping and the tally need anyway), the
       results down, and the f + 1 comparison and first-valid search in a C loop;
  (b)  pbft_accept_replies: the blocking form;
  (c)  pbft_accept_replies_device alone, HIP events around its chain.

The outputs are compared before anything is timed.  (a*) and (b) alternate; the outer time is a host clock around calls
that end in a synchronise; pinned host buffers.  Workloads, all canonical: 2,048 requests x 4 replicas = 8,192 replies
with the 8-byte result "awesome!" and with 1,024-byte results.  The condition on speed: (b)'s median is not above (a*)'s
by more than (a*)'s own min-max spread.
usage: python tools/accept_probe.py [--reps 30] [--requests 2048] [--out FILE.json]"""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DRIVER_SRC = os.path.join(ROOT, "tools", "accept", "accept_driver.cpp")
DRIVER_LIB = os.path.join(ROOT, "tools", "accept", "libaccept_driver.so")


def build_driver():
    from pbft_amd import native_build
    deps = [DRIVER_SRC, native_build.LIB] + native_build._headers()
    if native_build._stale(DRIVER_LIB, deps):
        cmd = ["g++"] + native_build.HOST_FLAGS + ["-shared", "-o", DRIVER_LIB, DRIVER_SRC,
                                                   "-L" + os.path.dirname(native_build.LIB), "-lpbft_verify",
                                                   "-Wl,-rpath,$ORIGIN/../../pbft_amd"]
        print("+", " ".join(cmd), flush=True)
        subprocess.run(cmd, cwd=ROOT, check=True)
    return DRIVER_LIB


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
    ap.add_argument("--requests", type=int, default=2048)
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    drv = ctypes.CDLL(build_driver())
    if a.build_only:
        return
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    drv.accept_driver_decode.restype = u64
    drv.accept_driver_decode.argtypes = [vp, vp, vp, u64, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp]
    drv.accept_driver_envelopes.restype = None
    drv.accept_driver_envelopes.argtypes = [u64, vp, vp, vp, vp, vp]
    drv.accept_driver_certify.restype = None
    drv.accept_driver_certify.argtypes = [u64, vp, vp, u32, vp, u32, vp, vp]
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    v = GpuBatchVerifier(0)
    lib = v._lib
    n_rep, need, view, q = 4, 2, 1, a.requests
    n = q * n_rep
    seeds = [hashlib.sha512(b"accept-probe-%d" % r).digest()[:32] for r in range(n_rep)]
    out = {"reps": a.reps, "requests": q, "replicas": n_rep, "n": n, "need": need, "workloads": {}}

    def pinned(shape, dtype=np.uint8):
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return torch.zeros(max(nbytes, 1), dtype=torch.uint8).pin_memory().numpy()[:nbytes].view(dtype).reshape(shape)

    def pin(x):
        p = pinned(x.shape, x.dtype)
        p[...] = x
        return p

    rng = np.random.default_rng(n)
    alpha = np.array([c for c in range(0x20, 0x7F) if c not in (0x22, 0x5C)], np.uint8)  # the canonical alphabet
    workloads = {"awesome_8B": [b"awesome!"] * q,
                 "results_1024B": [alpha[rng.integers(0, len(alpha), 1024)].tobytes() for _ in range(q)]}
    addrs = ["127.0.0.1:%d" % (8000 + i) for i in range(100)]
    cl_table = pin(np.frombuffer(b"".join(wire.client_field(c) for c in addrs), np.uint8).reshape(100, 64))
    pubs = []
    for name, results in workloads.items():
        # the replies: every replica signs every request with the library's own signer
        req = wire.pack_results(results, np.arange(1, q + 1), [addrs[i % 100] for i in range(q)])
        per = []
        for r in range(n_rep):
            pub = v.set_signing_seed(seeds[r], r)
            if len(pubs) < n_rep:
                pubs.append(pub.copy())
            stream, off, _, _, st = v.sign_replies(view, req)
            assert not st.any()
            per.append([stream[int(off[i]):int(off[i + 1])].tobytes() for i in range(q)])
        v.set_signing_seed(None)
        texts = [per[r][i] for i in range(q) for r in range(n_rep)]
        buf, off, ln = wire.pack_replies(texts)
        text_bytes = int(ln.sum())
        buf, off, ln = pin(buf), pin(off), pin(ln)
        ci = pin(np.repeat(np.arange(q, dtype=np.uint32) % 100, n_rep))
        keys = np.stack(pubs)
        assert v.set_keys(keys).all()
        v.accept_reserve(n), v.reserve(n), v.group_reserve(n)
        pid_table = pin(np.frombuffer(b"".join(wire.peer_id_b58(p.tobytes()) for p in pubs), np.uint8))
        env_cap, W, words = q + 64, 1, (n + 63) // 64

        # ---- (a*) ----
        res_off, res_len, rows = pinned(n, np.uint64), pinned(n, np.uint32), pinned((n, 64))
        R, S, key, vw, ts = pinned((n, 32)), pinned((n, 32)), pinned(n, np.uint16), pinned(n, np.uint64), pinned(n, np.uint64)
        dig, env, rec = pinned((n, 64)), pinned((n, 85)), pinned((n, 160))
        a_bits, a_idx, a_env = pinned(words, np.uint64), pinned(n, np.uint32), pinned((env_cap, 85))
        a_nenv, a_set, a_cnt = pinned(2, np.uint32), pinned((env_cap, W), np.uint64), pinned(env_cap, np.uint32)
        a_first, a_acc = pinned(env_cap, np.uint32), pinned(env_cap, np.uint32)
        d = {k: torch.zeros(s, dtype=torch.uint8, device=dev) for k, s in
             dict(rec=160 * n, bits=8 * words, idx=4 * n, env=85 * env_cap + 11, n_env=8, set=8 * env_cap * W,
                  cnt=4 * env_cap).items()}
        host = dict(rec=rec, bits=a_bits, idx=a_idx, env=a_env, n_env=a_nenv, set=a_set, cnt=a_cnt)
        host_t = {k: torch.from_numpy(x.view(np.uint8).reshape(-1)) for k, x in host.items()}
        s_a = torch.cuda.Stream(dev)

        def a_decode():
            kept = drv.accept_driver_decode(buf.ctypes.data, off.ctypes.data, ln.ctypes.data, n, pid_table.ctypes.data,
                                            n_rep, ci.ctypes.data, cl_table.ctypes.data, 100, res_off.ctypes.data,
                                            res_len.ctypes.data, rows.ctypes.data, R.ctypes.data, S.ctypes.data,
                                            key.ctypes.data, vw.ctypes.data, ts.ctypes.data)
            assert kept == n

        def a_digest():
            check(lib.pbft_reply_digests(n, rows.ctypes.data, buf.ctypes.data, text_bytes, res_off.ctypes.data,
                                         res_len.ctypes.data, dig.ctypes.data))

        def a_pack():
            drv.accept_driver_envelopes(n, key.ctypes.data, vw.ctypes.data, ts.ctypes.data, dig.ctypes.data,
                                        env.ctypes.data)
            check(lib.pbft_records_pack(R.ctypes.data, S.ctypes.data, key.ctypes.data, env.ctypes.data, 85, n,
                                        rec.ctypes.data))

        def a_device():
            with torch.cuda.stream(s_a):
                d["rec"].copy_(host_t["rec"], non_blocking=True)
                p = d["rec"].data_ptr()
                check(lib.pbft_group_envelopes_device(v._ctx, p + 64, 160, p + 150, 160, n, env_cap, d["idx"].data_ptr(),
                                                      d["env"].data_ptr(), d["n_env"].data_ptr(), s_a.cuda_stream))
                check(lib.pbft_verify_records_device(v._ctx, p, n, d["bits"].data_ptr(), s_a.cuda_stream))
                check(lib.pbft_tally_device(v._ctx, d["bits"].data_ptr(), p + 150, 160, d["idx"].data_ptr(), 4, n, env_cap,
                                            n_rep, 0, d["set"].data_ptr(), d["cnt"].data_ptr(), s_a.cuda_stream))
                for k in ("bits", "idx", "n_env", "set", "cnt"):
                    host_t[k].copy_(d[k], non_blocking=True)
                host_t["env"].copy_(d["env"][:85 * env_cap], non_blocking=True)
            s_a.synchronize()

        def a_certify():
            drv.accept_driver_certify(n, a_bits.ctypes.data, a_idx.ctypes.data, min(int(a_nenv[0]), env_cap),
                                      a_cnt.ctypes.data, need, a_first.ctypes.data, a_acc.ctypes.data)

        parts_a = (("c_loop_decode_reply_and_signer_rule", a_decode), ("pbft_reply_digests", a_digest),
                   ("c_loop_envelopes_and_pbft_records_pack", a_pack),
                   ("upload_group_verify_tally_download", a_device), ("c_loop_f_plus_1_and_first_valid", a_certify))

        def leg_a_star():
            for _, f in parts_a:
                f()

        # ---- (b) ----
        b_bits, b_heads, b_env = pinned(words, np.uint64), pinned(n, wire.AcceptHead), pinned((env_cap, 85))
        b_nenv, b_set, b_cnt = pinned(2, np.uint32), pinned((env_cap, W), np.uint64), pinned(env_cap, np.uint32)
        b_cert = pinned(env_cap, wire.AcceptCert)

        def leg_b():
            check(lib.pbft_accept_replies(v._ctx, buf.ctypes.data, text_bytes, off.ctypes.data, ln.ctypes.data,
                                          ci.ctypes.data, cl_table.ctypes.data, 100, n, need, env_cap,
                                          b_bits.ctypes.data, b_heads.ctypes.data, None, b_env.ctypes.data,
                                          b_nenv.ctypes.data, b_set.ctypes.data, b_cnt.ctypes.data, b_cert.ctypes.data))

        # ---- (c) ----
        d_in = [torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
                for x in (buf, off, ln, ci, cl_table)]
        c = {k: torch.zeros(s, dtype=torch.uint8, device=dev) for k, s in
             dict(rec=160 * n, heads=32 * n, bits=8 * words, idx=4 * n, env=85 * env_cap + 11, n_env=8,
                  set=8 * env_cap * W, cnt=4 * env_cap, cert=32 * env_cap).items()}
        s_c = torch.cuda.Stream(dev)
        p = [t.data_ptr() for t in d_in]

        def leg_c():
            v.accept_replies_device(p[0], text_bytes, p[1], p[2], p[4], 100, n, need, c["rec"].data_ptr(),
                                    c["heads"].data_ptr(), c["bits"].data_ptr(), env_cap, c["idx"].data_ptr(),
                                    c["env"].data_ptr(), c["n_env"].data_ptr(), c["set"].data_ptr(), c["cnt"].data_ptr(),
                                    c["cert"].data_ptr(), d_client_idx=p[3], stream=s_c.cuda_stream)

        # 1. outputs first
        leg_a_star()
        leg_b()
        ne = int(a_nenv[0])
        assert ne == q and list(b_nenv) == [q, 0] and list(a_nenv) == [q, 0]
        assert (a_bits == b_bits).all() and bin(int(a_bits[0])).count("1") == min(n, 64)
        assert (a_env == b_env).all() and (a_cnt == b_cnt).all() and (a_set == b_set).all()
        assert (a_first[:ne] == b_cert["first"][:ne]).all() and (a_acc[:ne] == b_cert["accepted"][:ne]).all()
        assert (b_cert["accepted"][:ne] == 1).all() and (b_cnt[:ne] == n_rep).all() and not b_heads["status"].any()
        leg_c()
        s_c.synchronize()
        assert (c["cert"].cpu().numpy().view(wire.AcceptCert) == b_cert).all()
        assert (c["bits"].cpu().numpy().view(np.uint64) == b_bits).all()
        res = {"text_bytes": text_bytes, "envelopes": ne,
               "checked": "(a*), (b) and (c): the same bits, envelopes, signer sets, counts, first-valid and accepted"}

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
        res["a_star_ms"] = stats(t_as)
        res["b_accept_replies_ms"] = stats(t_b)
        parts = {k: [] for k, _ in parts_a}
        for _ in range(a.reps):  # the parts of (a*), apart
            for k, f in parts_a:
                t0 = time.perf_counter()
                f()
                parts[k].append((time.perf_counter() - t0) * 1e3)
        res["a_star_parts_ms"] = {k: stats(x) for k, x in parts.items()}
        sa, sb = res["a_star_ms"], res["b_accept_replies_ms"]
        res["condition_b_not_above_a_star_by_more_than_its_spread"] = {
            "b_minus_a_star_median_ms": sb["median"] - sa["median"], "a_star_spread_ms": sa["max"] - sa["min"],
            "met": bool(sb["median"] - sa["median"] <= sa["max"] - sa["min"])}

        # 3. (c), the chain alone; and its first stage alone
        for what, call in (("c_device_chain_ms", leg_c),
                           ("c_decode_stage_alone_ms", lambda: v.decode_replies_device(
                               p[0], text_bytes, p[1], p[2], p[4], 100, n, c["rec"].data_ptr(), c["heads"].data_ptr(),
                               d_client_idx=p[3], stream=s_c.cuda_stream))):
            ms = []
            for r in range(a.reps + 3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                with torch.cuda.stream(s_c):
                    e0.record(s_c)
                    call()
                    e1.record(s_c)
                torch.cuda.synchronize()
                if r >= 3:
                    ms.append(e0.elapsed_time(e1))
            res[what] = stats(ms)
        out["workloads"][name] = res
    out["note"] = ("(a*), (b): wall clock of blocking calls on one host thread, pinned host buffers; (c): HIP events "
                   "around the kernels of one device call")
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    v.close()


if __name__ == "__main__":
    main()
