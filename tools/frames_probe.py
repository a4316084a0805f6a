#!/usr/bin/env python3
"""The GPU frame decoder at 2^20 canonical signed-vote frames of the config-#4 round (n = 256, UviBytes + JSON, as
pbft_wire_encode_votes writes them).
--part device: HIP events around pbft_wire_decode_frames_device, around pbft_verify_records_device of the records it
  wrote (comb + finish), and around a plain device-to-device copy that moves the decode kernel's algorithmic bytes
  (the 16-byte granules of the frames read + 184 bytes written per frame; the copy reads half of that and writes half),
  interleaved, medians.  floor_ms is that copy; the goal for the kernel is 2 x floor_ms.
--part host: votes/s of the blocking pbft_verify_frames from pinned host memory, next to pbft_wire_decode_votes +
  pbft_records_pack + pbft_verify_records on one thread and to pbft_verify_records alone on pre-decoded pinned records.
Every path's bitmap is checked first.
usage: python tools/frames_probe.py --part device|host [--reps R] [--log2n 20] [--out FILE.json]"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pinned(a):
    import torch
    return torch.from_numpy(a).pin_memory().numpy()


def main():
    import numpy as np
    import torch
    import bench
    from pbft_amd import FrameHead, GpuBatchVerifier, bitmap_to_bool, wire
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("device", "host"), required=True)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    n_sig = bench.N_REPLICAS
    n = 1 << a.log2n
    seeds = bench.key_seeds(n_sig)
    msg, key_idx = bench.envelopes(1, n // (2 * n_sig), n_sig)
    v = GpuBatchVerifier(0)
    R, S_good, pub = v.sign(seeds, key_idx, msg, bench.ENVELOPE)
    S, bad = bench.corrupt(S_good, bench.ADV_FRAC, bench.SEED)
    expect = np.ones(n, bool)
    expect[bad] = False
    assert v.set_keys(pub).all()
    kind = msg[:, 4].copy()
    view = msg[:, 5:13].copy().view(np.uint64).reshape(n)
    seq = msg[:, 13:21].copy().view(np.uint64).reshape(n)
    stream = wire.encode_votes(kind, view, seq, msg[:, 21:], key_idx.astype(np.uint32), np.concatenate([R, S], axis=1))
    off, flen, used = wire.frame_index(stream)
    assert len(off) == n and used == len(stream)
    granules = int((((off % 16) + flen + 15) // 16).sum())
    algo_bytes = 16 * granules + 184 * n
    out = {"part": a.part, "n": n, "n_signers": n_sig, "reps": a.reps, "stream_bytes": int(len(stream)),
           "bytes_per_frame": len(stream) / n, "algorithmic_bytes": algo_bytes}
    words = (n + 63) // 64
    if a.part == "device":
        pad = (-len(stream)) % 16
        dS = torch.from_numpy(np.concatenate([stream, np.zeros(pad, np.uint8)])).to(dev)
        dO, dL = torch.from_numpy(off.view(np.int64)).to(dev), torch.from_numpy(flen.view(np.int32)).to(dev)
        dRec = torch.zeros(n * 160, dtype=torch.uint8, device=dev)
        dHd = torch.zeros(n * 24, dtype=torch.uint8, device=dev)
        dB = torch.zeros(words, dtype=torch.int64, device=dev)
        src = torch.zeros(algo_bytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.zeros(algo_bytes // 2, dtype=torch.uint8, device=dev)
        v.reserve(n)
        st = torch.cuda.Stream(dev)

        def decode():
            v.decode_frames_device(dS.data_ptr(), len(stream), dO.data_ptr(), dL.data_ptr(), n_sig, n,
                                   dRec.data_ptr(), dHd.data_ptr(), stream=st.cuda_stream)

        def verify():
            check = v._lib.pbft_verify_records_device(v._ctx, dRec.data_ptr(), n, dB.data_ptr(), st.cuda_stream)
            assert check == 0
        for _ in range(3):
            decode()
            verify()
        torch.cuda.synchronize()
        heads = dHd.cpu().numpy().view(FrameHead)
        assert (heads["status"] == 0).all() and (heads["key_idx"] == key_idx).all() and (heads["seq"] == seq).all()
        assert (bitmap_to_bool(dB.cpu().numpy().view(np.uint64), n) == expect).all()
        t = {"decode_ms": [], "verify_ms": [], "copy_ms": []}
        for rep in range(a.reps + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                ev[0].record(st)
                decode()
                ev[1].record(st)
                verify()
                ev[2].record(st)
                dst.copy_(src)
                ev[3].record(st)
            torch.cuda.synchronize()
            if rep:
                for k, name in enumerate(("decode_ms", "verify_ms", "copy_ms")):
                    t[name].append(ev[k].elapsed_time(ev[k + 1]))
        med = {k: float(np.median(x)) for k, x in t.items()}
        out.update(med)
        out.update({"decode_ms_min": float(min(t["decode_ms"])), "floor_ms": med["copy_ms"],
                    "copy_GBps": algo_bytes / med["copy_ms"] / 1e6, "decode_GBps": algo_bytes / med["decode_ms"] / 1e6,
                    "decode_over_floor": med["decode_ms"] / med["copy_ms"],
                    "decode_share_of_verify": med["decode_ms"] / med["verify_ms"],
                    "decode_frames_per_s": n / med["decode_ms"] * 1e3,
                    "note": "HIP events on the launch stream; verify = comb + finish of the decoded records"})
    else:
        lib = v._lib
        h_stream, h_off, h_len = pinned(stream), pinned(off), pinned(flen)
        h_bm, h_heads = pinned(np.zeros(words, np.uint64)), pinned(np.zeros(n, FrameHead).view(np.uint8))

        def frames():
            rc = lib.pbft_verify_frames(v._ctx, h_stream.ctypes.data, len(stream), h_off.ctypes.data, h_len.ctypes.data,
                                        None, n_sig, n, h_bm.ctypes.data, h_heads.ctypes.data, None)
            assert rc == 0, lib.pbft_last_error()
            return h_bm
        st8 = np.zeros(n, np.uint8)
        hR, hS = np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8)
        hK, hM = np.zeros(n, np.uint16), np.zeros((n, 85), np.uint8)
        h_rec = pinned(np.zeros((n, 160), np.uint8))
        h_bm2 = pinned(np.zeros(words, np.uint64))
        nf, nr, cons = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()

        def host_decode():
            rc = lib.pbft_wire_decode_votes(h_stream.ctypes.data, len(stream), n_sig, n, n, st8.ctypes.data,
                                            hR.ctypes.data, hS.ctypes.data, hK.ctypes.data, hM.ctypes.data, None, None,
                                            None, ctypes.byref(nf), ctypes.byref(nr), ctypes.byref(cons))
            assert rc == 0 and nr.value == n
            assert lib.pbft_records_pack(hR.ctypes.data, hS.ctypes.data, hK.ctypes.data, hM.ctypes.data, 85, n,
                                         h_rec.ctypes.data) == 0
            assert lib.pbft_verify_records(v._ctx, h_rec.ctypes.data, n, h_bm2.ctypes.data) == 0
            return h_bm2

        def records():
            assert lib.pbft_verify_records(v._ctx, h_rec.ctypes.data, n, h_bm2.ctypes.data) == 0
            return h_bm2
        paths = (("verify_frames", frames), ("decode_votes_pack_verify_records", host_decode),
                 ("verify_records_predecoded", records))
        for name, fn in paths:  # warm (the staging grows), and check
            for _ in range(2):
                bm = fn()
            assert (bitmap_to_bool(bm.copy(), n) == expect).all(), name
        assert (h_heads.view(FrameHead)["status"] == 0).all()
        t = {name: [] for name, _ in paths}
        for rep in range(a.reps):
            for name, fn in paths:  # interleaved
                t0 = time.perf_counter()
                fn()
                t[name].append(time.perf_counter() - t0)
        for name, _ in paths:
            s = float(np.median(t[name]))
            out[name] = {"ms_median": s * 1e3, "ms_min": float(min(t[name])) * 1e3, "votes_per_s": n / s}
        out["passes_50M_votes_per_s"] = out["verify_frames"]["votes_per_s"] >= 50e6
        out["note"] = "wall clock of blocking calls on one host thread; inputs and outputs in pinned host memory"
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    v.close()


if __name__ == "__main__":
    main()
