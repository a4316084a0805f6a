#!/usr/bin/env python3
"""Cost of the frame index made on the GPU (pbft_wire_index_streams_device) on the stream of 2^20 canonical vote
frames of the config-#4 round (n = 256 signers), split into S = 255, 3 and 1 connection segments.
--part device: HIP events around the index kernels, around decode_frames_kernel of the index they wrote and around
  pbft_verify_records_device of the decoded records (comb + finish), interleaved over the cases, medians with
  min-max; the tile sizes of --tiles at S = 3; and one adversarial case, S = 255 with one connection that sends only
  zero-length frames.
--part host: pbft_wire_frame_index on the same stream in pinned host memory, one thread; then the whole calls: the
  host index of every segment, the concatenation, the peer expansion and pbft_verify_frames_tally together, next to
  pbft_verify_streams_tally, wall clock, and the bytes each moves per vote in each direction.  Both whole calls run
  without a peer array, so that every vote stays valid and the bits are known; the old path still expands one, which
  is what its caller has to do, but does not copy it up.
Every output is checked against the host index / the expected bits before anything is timed.
usage: python tools/index_probe.py [--part device|host|all] [--reps R] [--log2n 20] [--tiles 4096,8192,16384]
                                   [--out FILE.json]"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPLITS = (255, 3, 1)


def pinned(a):
    import torch
    return torch.from_numpy(a).pin_memory().numpy()


def stats(x):
    import numpy as np
    x = np.array(x)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max())}


def main():
    import numpy as np
    import torch
    import bench
    from pbft_amd import FrameHead, GpuBatchVerifier, SegHead, bitmap_to_bool, wire
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("device", "host", "all"), default="all")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--tiles", default="4096,8192,16384")
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
    Sg, bad = bench.corrupt(S_good, bench.ADV_FRAC, bench.SEED)
    expect = np.ones(n, bool)
    expect[bad] = False
    assert v.set_keys(pub).all()
    lib = v._lib
    kind = msg[:, 4].copy()
    view = msg[:, 5:13].copy().view(np.uint64).reshape(n)
    seq = msg[:, 13:21].copy().view(np.uint64).reshape(n)
    stream = wire.encode_votes(kind, view, seq, msg[:, 21:], key_idx.astype(np.uint32), np.concatenate([R, Sg], axis=1))
    off, flen, used = wire.frame_index(stream)
    assert len(off) == n and used == len(stream)
    nbytes = len(stream)
    words, W = (n + 63) // 64, (n_sig + 63) // 64
    out = {"n": n, "n_signers": n_sig, "stream_bytes": int(nbytes), "reps": a.reps}

    def segments(S):
        """S runs of whole frames, back to back: (seg_off, seg_len, first frame of each)."""
        first = np.arange(S + 1, dtype=np.int64) * n // S
        start = np.concatenate([off - 2, [nbytes]]).astype(np.uint64)[first]  # (two-byte varints)
        return start[:-1].copy(), (start[1:] - start[:-1]).copy(), first

    if a.part in ("device", "all"):
        v.reserve(n)
        v.index_reserve(nbytes, 255)
        st = torch.cuda.Stream(dev)
        d_stream = torch.from_numpy(np.concatenate([stream, np.zeros((-nbytes) % 16, np.uint8)])).to(dev)
        d = {"off": torch.zeros(n, dtype=torch.int64, device=dev), "len": torch.zeros(n, dtype=torch.int32, device=dev),
             "peer": torch.zeros(n, dtype=torch.int16, device=dev), "nfr": torch.zeros(2, dtype=torch.int32, device=dev),
             "rec": torch.zeros(n * 160, dtype=torch.uint8, device=dev),
             "hd": torch.zeros(n * 24, dtype=torch.uint8, device=dev), "B": torch.zeros(words, dtype=torch.int64, device=dev)}

        def case(S, tile=0, src=d_stream, cap=n, total=n):
            so, sl, first = segments(S)
            t = {"so": torch.from_numpy(so.view(np.int64)).to(dev), "sl": torch.from_numpy(sl.view(np.int64)).to(dev),
                 "sp": torch.from_numpy((np.arange(S) % n_sig).astype(np.int16)).to(dev),
                 "heads": torch.zeros(S * 24, dtype=torch.uint8, device=dev)}

            def index():
                v.set_option(v.OPT_INDEX_TILE, tile)
                v.index_streams_device(src.data_ptr(), nbytes, t["so"].data_ptr(), t["sl"].data_ptr(), S, cap,
                                       d["off"].data_ptr(), d["len"].data_ptr(), t["heads"].data_ptr(),
                                       d["nfr"].data_ptr(), d_seg_peer=t["sp"].data_ptr(), d_peer=d["peer"].data_ptr(),
                                       stream=st.cuda_stream)
            index()
            torch.cuda.synchronize()
            assert d["nfr"].cpu().numpy().view(np.uint32).tolist() == [total, max(0, total - cap)], (S, tile)
            if total == n:  # the plain stream: the host index, and every segment consumed whole
                assert (d["off"].cpu().numpy().view(np.uint64) == off).all(), (S, tile)
                assert (d["len"].cpu().numpy().view(np.uint32) == flen).all(), (S, tile)
                h = t["heads"].cpu().numpy().view(SegHead)
                assert (h["consumed"] == sl).all() and not h["status"].any() and (h["first"] == first[:-1]).all()
                assert (d["peer"].cpu().numpy().view(np.uint16) == np.repeat(np.arange(S) % n_sig, np.diff(first))).all()
            return index, t

        def decode():
            v.decode_frames_device(d_stream.data_ptr(), nbytes, d["off"].data_ptr(), d["len"].data_ptr(), n_sig, n,
                                   d["rec"].data_ptr(), d["hd"].data_ptr(), stream=st.cuda_stream)

        def verify():
            assert lib.pbft_verify_records_device(v._ctx, d["rec"].data_ptr(), n, d["B"].data_ptr(), st.cuda_stream) == 0
        cases = {"S=%d" % S: case(S) for S in SPLITS}
        for tile in [int(x) for x in a.tiles.split(",") if x]:
            cases["S=3 tile=%d" % tile] = case(3, tile)
        # one of 255 connections sends only zero-length frames: its bytes become that many frames
        so, sl, _ = segments(255)
        hostile = stream.copy()
        hostile[int(so[100]):int(so[100] + sl[100])] = 0
        d_hostile = torch.from_numpy(np.concatenate([hostile, np.zeros((-nbytes) % 16, np.uint8)])).to(dev)
        n_hostile = n - (n * 101 // 255 - n * 100 // 255) + int(sl[100])
        cases["S=255 one connection of zero-length frames"] = case(255, src=d_hostile, total=n_hostile)
        for _ in range(2):  # warm, and check the chain on the plain index
            cases["S=1"][0]()
            decode()
            verify()
        torch.cuda.synchronize()
        assert (bitmap_to_bool(d["B"].cpu().numpy().view(np.uint64), n) == expect).all()
        assert not d["hd"].cpu().numpy().view(FrameHead)["status"].any()
        res = {name: {"index_ms": [], "decode_ms": [], "verify_ms": []} for name in cases}
        for rep in range(a.reps + 1):
            for name, (index, _) in cases.items():  # interleaved
                plain = name in ("S=255", "S=3", "S=1")
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                torch.cuda.synchronize()
                with torch.cuda.stream(st):
                    ev[0].record(st)
                    index()
                    ev[1].record(st)
                    if plain:
                        decode()
                    ev[2].record(st)
                    if plain:
                        verify()
                    ev[3].record(st)
                torch.cuda.synchronize()
                if rep:
                    res[name]["index_ms"].append(ev[0].elapsed_time(ev[1]))
                    if plain:
                        res[name]["decode_ms"].append(ev[1].elapsed_time(ev[2]))
                        res[name]["verify_ms"].append(ev[2].elapsed_time(ev[3]))
        v.set_option(v.OPT_INDEX_TILE, 0)
        dev_out = {"note": "HIP events on the launch stream; index = the kernels of pbft_wire_index_streams_device; "
                           "decode = decode_frames_kernel; verify = comb + finish of the decoded records"}
        for name, r in res.items():
            dev_out[name] = {k: stats(x) for k, x in r.items() if x}
            if r["decode_ms"]:
                dev_out[name]["index_over_decode"] = dev_out[name]["index_ms"]["median"] / \
                    dev_out[name]["decode_ms"]["median"]
        out["device"] = dev_out
    if a.part in ("host", "all"):
        h_stream = pinned(stream)
        h_off, h_len = pinned(np.zeros(n, np.uint64)), pinned(np.zeros(n, np.uint32))
        h_peer = pinned(np.zeros(n, np.uint16))
        h_bm, h_heads = pinned(np.zeros(words, np.uint64)), pinned(np.zeros(n, FrameHead).view(np.uint8))
        h_env, h_n = pinned(np.zeros((n_env, 85), np.uint8)), pinned(np.zeros(2, np.uint32))
        h_sets, h_cnt = pinned(np.zeros((n_env, W), np.uint64)), pinned(np.zeros(n_env, np.uint32))
        nf, cons = ctypes.c_uint64(), ctypes.c_uint64()

        def walk():
            rc = lib.pbft_wire_frame_index(h_stream.ctypes.data, nbytes, n, h_off.ctypes.data, h_len.ctypes.data,
                                           ctypes.byref(nf), ctypes.byref(cons))
            assert rc == 0 and nf.value == n
        walk()
        assert (h_off == off).all() and (h_len == flen).all()
        t_walk = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            walk()
            t_walk.append(time.perf_counter() - t0)
        host = {"note": "wall clock of blocking calls on one host thread; inputs and outputs in pinned host memory",
                "host_walk_ms": stats([x * 1e3 for x in t_walk])}
        paths = {}
        for S in SPLITS:
            so, sl, first = segments(S)
            sp = (np.arange(S) % n_sig).astype(np.uint16)
            h_seg = pinned(np.zeros(S, SegHead).view(np.uint8))
            h_nfr = pinned(np.zeros(2, np.uint32))

            def old(so=so, sl=sl, sp=sp, S=S):
                at = 0
                for s in range(S):  # the walk per connection, its offsets made absolute, its peer expanded
                    rc = lib.pbft_wire_frame_index(h_stream.ctypes.data + int(so[s]), int(sl[s]), n - at,
                                                   h_off.ctypes.data + 8 * at, h_len.ctypes.data + 4 * at,
                                                   ctypes.byref(nf), ctypes.byref(cons))
                    assert rc == 0
                    k = nf.value
                    h_off[at:at + k] += so[s]
                    h_peer[at:at + k] = sp[s]
                    at += k
                assert at == n
                rc = lib.pbft_verify_frames_tally(v._ctx, h_stream.ctypes.data, nbytes, h_off.ctypes.data,
                                                  h_len.ctypes.data, None, n_sig, n, n_env, h_bm.ctypes.data,
                                                  h_heads.ctypes.data, None, h_env.ctypes.data, h_n.ctypes.data,
                                                  h_sets.ctypes.data, h_cnt.ctypes.data)
                assert rc == 0, lib.pbft_last_error()

            def new(so=so, sl=sl, S=S, h_seg=h_seg, h_nfr=h_nfr):
                rc = lib.pbft_verify_streams_tally(v._ctx, h_stream.ctypes.data, nbytes, so.ctypes.data, sl.ctypes.data,
                                                   None, S, n_sig, n, n_env, h_bm.ctypes.data, h_heads.ctypes.data, None,
                                                   h_env.ctypes.data, h_n.ctypes.data, h_sets.ctypes.data,
                                                   h_cnt.ctypes.data, h_seg.ctypes.data, h_nfr.ctypes.data, None, None)
                assert rc == 0, lib.pbft_last_error()
            keep = {}
            for name, fn in (("old", old), ("new", new)):  # warm (the staging grows), and check
                for _ in range(2):
                    fn()
                assert (bitmap_to_bool(h_bm.copy(), n) == expect).all(), (S, name)
                keep[name] = [x.copy() for x in (h_bm, h_heads, h_env, h_n, h_sets, h_cnt)]
            assert all((x == y).all() for x, y in zip(keep["old"], keep["new"])), S
            assert h_nfr.tolist() == [n, 0] and (h_seg.view(SegHead)["consumed"] == sl).all()
            paths[S] = (old, new)
        t = {(S, k): [] for S in SPLITS for k in ("old", "new")}
        for rep in range(a.reps):
            for S in SPLITS:  # interleaved
                for k, fn in zip(("old", "new"), paths[S]):
                    t0 = time.perf_counter()
                    fn()
                    t[(S, k)].append(time.perf_counter() - t0)
        per_env = n_env * (85 + 8 * W + 4) + 8
        for S in SPLITS:
            o, w = stats([x * 1e3 for x in t[(S, "old")]]), stats([x * 1e3 for x in t[(S, "new")]])
            host["S=%d" % S] = {
                "host_index_then_verify_frames_tally_ms": o, "verify_streams_tally_ms": w,
                "new_over_old": w["median"] / o["median"],
                "bytes_up_per_vote": {"old": nbytes / n + 12, "old_with_peers": nbytes / n + 14,
                                      "new": nbytes / n + 16 * S / n, "new_with_peers": nbytes / n + 18 * S / n},
                "bytes_back_per_vote": {"old": 24 + 1 / 8 + per_env / n,
                                        "new": 24 + 1 / 8 + per_env / n + (24 * S + 8) / n}}
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
