#!/usr/bin/env python3
"""Cost of pbft_replica_push_streams on the 2^20-vote config-#4 round (n = 256 signers, 2,048 seqs, a Prepare and a
Commit of every signer per seq) as 256 connection streams, one per signer.
--part device: HIP events around the kernels of pbft_admit_device, beside decode_frames_kernel and comb + finish
  (pbft_verify_records_device) of the same run, and a device-to-device copy of the 27 bytes per row the admission pass
  reads and writes (24-byte head in, class byte and key index out); interleaved, medians with min-max.
--part host: the whole call on a fresh replica per repeat, wall clock, against the only other way to ingest these
  bytes into a replica -- 256 pbft_replica_push_frames calls and the forced flush -- and beside
  pbft_verify_streams_tally on the same bytes (its floor: the call adds the admission kernels, a second tally and the
  host application of 4,096 x 2 signer sets); the share of the call's host time spent applying the sets.
Every output is checked against the host path (counters and events of the two replicas) before anything is timed.
usage: python tools/replica_streams_probe.py [--part device|host|all] [--reps R] [--log2n 20] [--out FILE.json]"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(x):
    import numpy as np
    x = np.array(x)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max())}


def main():
    import numpy as np
    import torch
    import bench
    from pbft_amd import AdmitResidue, FrameHead, GpuBatchVerifier, SegHead, wire
    from test_replica_streams import SAME, Event, SegHead as CSegHead, Stats, StreamsStats, bind
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
    msg, key_idx = bench.envelopes(1, n // (2 * n_sig), n_sig)
    v = GpuBatchVerifier(0)
    R, S_good, pub = v.sign(bench.key_seeds(n_sig), key_idx, msg, bench.ENVELOPE)
    Sg, bad = bench.corrupt(S_good, bench.ADV_FRAC, bench.SEED)
    assert v.set_keys(pub).all()
    lib = bind(v._lib)
    order = np.argsort(key_idx, kind="stable")  # one connection per signer: its votes in round order
    kind = msg[order, 4].copy()
    view = msg[order, 5:13].copy().view(np.uint64).reshape(n)
    seq = msg[order, 13:21].copy().view(np.uint64).reshape(n)
    assert (view == 1).all() and seq.min() >= 1 and seq.max() <= 4096
    stream = wire.encode_votes(kind, view, seq, msg[order, 21:], key_idx[order].astype(np.uint32),
                               np.concatenate([R, Sg], axis=1)[order])
    off, flen, used = wire.frame_index(stream)
    assert len(off) == n and used == len(stream)
    nbytes = len(stream)
    first = np.arange(n_sig + 1, dtype=np.int64) * (n // n_sig)
    start = np.concatenate([off - 2, [nbytes]]).astype(np.uint64)[first]  # (two-byte varints)
    seg_off, seg_len = start[:-1].copy(), (start[1:] - start[:-1]).copy()
    seg_peer = np.arange(n_sig, dtype=np.uint16)
    out = {"n": n, "n_signers": n_sig, "segments": n_sig, "stream_bytes": int(nbytes), "reps": a.reps,
           "forged": int(len(bad))}

    if a.part in ("device", "all"):
        v.reserve(n)
        v.admit_reserve(4096, n_sig, n)
        st = torch.cuda.Stream(dev)
        d_stream = torch.from_numpy(np.concatenate([stream, np.zeros((-nbytes) % 16, np.uint8)])).to(dev)
        d_off, d_len = torch.from_numpy(off.view(np.int64)).to(dev), torch.from_numpy(flen.view(np.int32)).to(dev)
        d_peer = torch.from_numpy(key_idx[order].astype(np.int16)).to(dev)
        words = (n + 63) // 64
        d = {k: torch.zeros(b, dtype=torch.uint8, device=dev)
             for k, b in (("rec", n * 160), ("hd", n * 24), ("cls", n), ("counts", 32), ("clean", 8 * words),
                          ("res", 16 * 4096), ("nres", 8), ("B", 8 * words), ("a", 27 * n), ("b", 27 * n))}

        def decode():
            v.decode_frames_device(d_stream.data_ptr(), nbytes, d_off.data_ptr(), d_len.data_ptr(), n_sig, n,
                                   d["rec"].data_ptr(), d["hd"].data_ptr(), d_peer=d_peer.data_ptr(),
                                   stream=st.cuda_stream)

        def admit():
            v.admit_device(d["hd"].data_ptr(), d["rec"].data_ptr(), n, 1, 0, 4096, n_sig, 4096, d["cls"].data_ptr(),
                           d["counts"].data_ptr(), d["clean"].data_ptr(), d["res"].data_ptr(), d["nres"].data_ptr(),
                           d_off=d_off.data_ptr(), d_len=d_len.data_ptr(), stream=st.cuda_stream)

        def verify():
            assert lib.pbft_verify_records_device(v._ctx, d["rec"].data_ptr(), n, d["B"].data_ptr(), st.cuda_stream) == 0
        for _ in range(2):
            decode(), admit(), verify()
        torch.cuda.synchronize()
        assert d["counts"].cpu().numpy().view(np.uint32).tolist() == [n, 0, 0, 0, 0, 0, 0, 0]
        assert not d["nres"].cpu().numpy().any() and (d["clean"].cpu().numpy() == 0xFF).all()
        assert not d["hd"].cpu().numpy().view(FrameHead)["status"].any() and AdmitResidue.itemsize == 16
        res = {"decode_ms": [], "admit_ms": [], "verify_ms": [], "copy_27B_per_row_ms": []}
        for rep in range(a.reps + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                ev[0].record(st)
                decode()
                ev[1].record(st)
                admit()
                ev[2].record(st)
                verify()
                ev[3].record(st)
                d["b"].copy_(d["a"])
                ev[4].record(st)
            torch.cuda.synchronize()
            if rep:
                for k, i in (("decode_ms", 0), ("admit_ms", 1), ("verify_ms", 2), ("copy_27B_per_row_ms", 3)):
                    res[k].append(ev[i].elapsed_time(ev[i + 1]))
        dev_out = {k: stats(x) for k, x in res.items()}
        dev_out["admit_over_copy"] = dev_out["admit_ms"]["median"] / dev_out["copy_27B_per_row_ms"]["median"]
        dev_out["note"] = ("HIP events on the launch stream; admit = the five kernels of pbft_admit_device (window 4096, "
                           "every row clean); copy = a device-to-device copy of 27 bytes per row")
        out["device"] = dev_out

    if a.part in ("host", "all"):
        from replica_sim import lib as replica_lib
        replica_lib()
        keys = pub.tobytes()
        stream_p = torch.from_numpy(stream.copy()).pin_memory().numpy()

        def replica():
            r = ctypes.c_void_p()
            assert lib.pbft_replica_create(v._ctx, n_sig, 0, keys, ctypes.byref(r)) == 0
            assert lib.pbft_replica_reserve_streams(r, nbytes, n_sig, n, n_env, 4096) == 0
            return r

        def counters(r):
            s = Stats()
            lib.pbft_replica_get_stats(r, ctypes.byref(s))
            return {k: getattr(s, k) for k in SAME}

        ev, ne = (Event * 8192)(), ctypes.c_uint32()

        def old(r):
            used, x, y = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
            assert lib.pbft_replica_flush(r, 1, ev, 8192, ctypes.byref(ne)) == 0
            for s in range(n_sig):
                buf = (ctypes.c_char * int(seg_len[s])).from_buffer(stream_p, int(seg_off[s]))
                assert lib.pbft_replica_push_frames(r, s, buf, int(seg_len[s]), ctypes.byref(used), ctypes.byref(x),
                                                    ctypes.byref(y)) == 0 and used.value == seg_len[s]
            assert lib.pbft_replica_flush(r, 1, ev, 8192, ctypes.byref(ne)) == 0

        heads = (CSegHead * n_sig)()

        def new(r):
            x, y = ctypes.c_uint64(), ctypes.c_uint64()
            rc = lib.pbft_replica_push_streams(r, stream_p.ctypes.data, nbytes, seg_off.ctypes.data, seg_len.ctypes.data,
                                               seg_peer.ctypes.data, n_sig, heads, ctypes.byref(x), ctypes.byref(y), ev,
                                               8192, ctypes.byref(ne))
            assert rc == 0 and x.value == n, (rc, x.value, y.value)

        words, W = (n + 63) // 64, (n_sig + 63) // 64
        t_bm, t_heads = np.zeros(words, np.uint64), np.zeros(n, FrameHead)
        t_env, t_n = np.zeros((n_env, 85), np.uint8), np.zeros(2, np.uint32)
        t_sets, t_cnt = np.zeros((n_env, W), np.uint64), np.zeros(n_env, np.uint32)
        t_seg, t_nfr = np.zeros(n_sig, SegHead), np.zeros(2, np.uint32)

        def floor(_r=None):
            rc = lib.pbft_verify_streams_tally(v._ctx, stream_p.ctypes.data, nbytes, seg_off.ctypes.data,
                                               seg_len.ctypes.data, seg_peer.ctypes.data, n_sig, n_sig, n, n_env,
                                               t_bm.ctypes.data, t_heads.ctypes.data, None, t_env.ctypes.data,
                                               t_n.ctypes.data, t_sets.ctypes.data, t_cnt.ctypes.data,
                                               t_seg.ctypes.data, t_nfr.ctypes.data, None, None)
            assert rc == 0, lib.pbft_last_error()

        ra = replica()  # warm, and check the two paths against each other (a context serves one replica at a time)
        old(ra)
        want = counters(ra)
        lib.pbft_replica_destroy(ra)
        rb = replica()
        new(rb)
        floor()
        assert counters(rb) == want and want["accepted"] == n - len(bad) and want["live_windows"] == n_env // 2
        assert want["rejected_sig"] == len(bad) and int(t_cnt.sum()) == n - len(bad)
        ss = StreamsStats()
        lib.pbft_replica_get_streams_stats(rb, ctypes.byref(ss))
        assert ss.calls_device == 1 and ss.clean_rows == n and ss.residue_rows == 0 and ss.envelopes == n_env
        lib.pbft_replica_destroy(rb)
        t = {"push_frames_x256_then_flush_ms": [], "push_streams_ms": [], "verify_streams_tally_ms": [],
             "apply_sets_ms": [], "front_ms": []}
        for _ in range(a.reps):
            for name, fn in (("push_frames_x256_then_flush_ms", old), ("push_streams_ms", new),
                             ("verify_streams_tally_ms", floor)):  # interleaved, a fresh replica each
                r = replica()
                t0 = time.perf_counter()
                fn(r)
                t[name].append((time.perf_counter() - t0) * 1e3)
                if fn is new:
                    lib.pbft_replica_get_streams_stats(r, ctypes.byref(ss))
                    t["apply_sets_ms"].append(ss.apply_sets_ns * 1e-6)
                    t["front_ms"].append(ss.front_ns * 1e-6)
                lib.pbft_replica_destroy(r)
        host = {k: stats(x) for k, x in t.items()}
        m = {k: host[k]["median"] for k in host}
        host["push_streams_over_push_frames"] = m["push_streams_ms"] / m["push_frames_x256_then_flush_ms"]
        host["push_streams_over_verify_streams_tally"] = m["push_streams_ms"] / m["verify_streams_tally_ms"]
        host["apply_sets_share_of_call"] = m["apply_sets_ms"] / m["push_streams_ms"]
        host["votes_per_s"] = {"push_frames": n / m["push_frames_x256_then_flush_ms"] * 1e3,
                               "push_streams": n / m["push_streams_ms"] * 1e3}
        host["note"] = ("wall clock of blocking calls on one host thread, a fresh replica per call (creation not timed); "
                        "front = the GPU chain with its copies; apply_sets = the signer sets applied to the windows")
        out["host"] = host
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    v.close()


if __name__ == "__main__":
    main()
