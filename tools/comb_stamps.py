#!/usr/bin/env python3
"""Phase stamps of comb_kernel waves (diagnostic build: tools/build_variant.sh stamps -DPBFT_COMB_STAMPS=1) at the
131k shard and at 2^20 (attribute the shard's stalls before trying another kernel shape).

Per size: the in-kernel clock (delta s_memtime / delta s_memrealtime x 100 MHz, median over waves), and per wave the
shader cycles of its phases -- hash + recoding, gather waits (vmcnt(0) before each step's entry read), LDS waits
(lgkmcnt(0)), the rest of the steps (arithmetic) -- plus the spread of wave start / end times across the launch
(realtime, so comparable across CUs) and the waves per SIMD that were live.  Then the attribution of the time in which
a SIMD has fewer than 4 waves resident (a sweep over each SIMD's wave intervals) and of each wave's time from its
start to its first table entry (hash + recoding, then the first gather's vmcnt wait), both as shares of the launch.
usage: python tools/comb_stamps.py build/ab/libpbft_stamps.so [sizes...]"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    lib_path = sys.argv[1]
    sizes = [int(x) for x in sys.argv[2:]] or [131072, 1 << 20]
    os.environ["PBFT_VERIFY_LIB"] = os.path.abspath(lib_path)  # read by pbft_amd._lib at import
    import torch
    import bench
    torch.cuda.set_device(0)
    from pbft_amd import GpuBatchVerifier, _lib
    lib = _lib.load()
    assert os.path.samefile(lib._name, lib_path), lib._name
    lib.pbft_debug_comb_stamps.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    seeds = bench.key_seeds(256)
    msg, key_idx = bench.envelopes(1, 2048, 256)
    v = GpuBatchVerifier(0)
    R, S, pub = v.sign(seeds, key_idx, msg, 85)
    assert v.set_keys(pub).all()
    dev = torch.device("cuda", 0)
    d = bench.to_device(torch, dev, R, S, key_idx, msg)
    st = torch.cuda.Stream(dev)
    for n in sizes:
        for _ in range(30):  # warm: the clock settles under load
            v.verify_device(d["R"].data_ptr(), d["S"].data_ptr(), d["K"].data_ptr(), d["M"].data_ptr(), 85, 85, n,
                            d["B"].data_ptr(), st.cuda_stream)
        st.synchronize()
        waves = (n + 63) // 64
        buf = np.zeros((min(waves, 16384), 8), np.uint64)
        assert lib.pbft_debug_comb_stamps(buf.ctypes.data, len(buf)) == 0
        if os.environ.get("PBFT_STAMPS_DUMP"):  # the raw stamps, for other analyses
            np.save(os.path.join(os.environ["PBFT_STAMPS_DUMP"], f"comb_stamps_{n}.npy"), buf)
        b = buf.astype(np.float64)
        life = b[:, 4] - b[:, 0]
        rt = (b[:, 5] - b[:, 1])
        clk = np.median(life / np.maximum(rt, 1)) * 0.1  # GHz (realtime ticks at 100 MHz)
        hash_ = b[:, 2] - b[:, 0]
        wait = (buf[:, 3] & np.uint64(0xFFFFFFFF)).astype(np.float64)
        first = (buf[:, 3] >> np.uint64(32)).astype(np.float64)  # the first step's share of the vmcnt waits
        lgkm = b[:, 6]
        rest = life - hash_ - wait - lgkm
        t0 = b[:, 1].min()
        start = (b[:, 1] - t0) / 100.0  # us
        end = (b[:, 5] - t0) / 100.0
        hw = (buf[:, 7] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        xcc = ((buf[:, 7] >> np.uint64(32)) & np.uint64(0xF)).astype(np.int64)
        simd = (hw >> 4) & 3
        cu = (hw >> 8) & 15
        sh = (hw >> 12) & 1
        se = (hw >> 13) & 3
        sid = (((xcc * 4 + se) * 2 + sh) * 16 + cu) * 4 + simd      # a SIMD of the chip
        cuid = sid >> 2
        _, inv_s, cnt_s = np.unique(sid, return_inverse=True, return_counts=True)
        _, inv_c, cnt_c = np.unique(cuid, return_inverse=True, return_counts=True)
        per_simd = cnt_s[inv_s]
        print(f"  placement: {len(cnt_c)} CUs, {len(cnt_s)} SIMDs used; waves per CU "
              + " ".join(f"{k}:{int((cnt_c == k).sum())}" for k in sorted(set(cnt_c.tolist())))
              + "; waves per SIMD " + " ".join(f"{k}:{int((cnt_s == k).sum())}" for k in sorted(set(cnt_s.tolist()))))
        for k in sorted(set(per_simd.tolist())):
            m = per_simd == k
            print(f"    waves on a SIMD shared by {k}: {int(m.sum())} waves, lifetime mean {life[m].mean():.0f} cyc, "
                  f"end mean {((b[m, 5] - b[:, 1].min()) / 100).mean():.1f} us")
        # waves live at each moment: sample at 200 points of the launch
        ts = np.linspace(0, end.max(), 200)
        live = np.array([((start <= t) & (end > t)).sum() for t in ts])
        print(f"== {n} signatures, {waves} waves: in-kernel clock {clk:.3f} GHz, launch span {end.max():.1f} us "
              f"(first wave end {end.min():.1f} us, last wave start {start.max():.1f} us)")
        for name, x in (("lifetime", life), ("hash+recode", hash_), ("gather vmcnt wait", wait),
                        ("LDS lgkmcnt wait", lgkm), ("steps other", rest)):
            print(f"  {name:18s} mean {x.mean():9.0f} cyc  p10 {np.percentile(x, 10):9.0f}  p90 "
                  f"{np.percentile(x, 90):9.0f}  ({100 * x.mean() / life.mean():5.1f} % of lifetime)")
        print(f"  wave start us: p0 {start.min():.1f} p50 {np.median(start):.1f} p90 {np.percentile(start, 90):.1f} "
              f"max {start.max():.1f}; end us: min {end.min():.1f} p10 {np.percentile(end, 10):.1f} p50 "
              f"{np.median(end):.1f} p90 {np.percentile(end, 90):.1f} max {end.max():.1f}")
        print(f"  live waves over the launch (200 samples): max {live.max()}, mean {live.mean():.0f} "
              f"(= {live.mean() / 1024:.2f} per SIMD), quartiles of time: "
              + " ".join(f"{live[i * 50:(i + 1) * 50].mean():.0f}" for i in range(4)))
        attribution(buf, sid, clk)
    v.close()


def attribution(buf, sid, clk):
    """Per SIMD: the time of the launch with k < 4 waves resident (realtime ticks of 10 ns, the launch taken from the
    first wave start to the last wave end of the chip), split into the lead-in before the SIMD's first wave, the gaps
    between its first start and its last end, and the tail after its last wave; and per wave the start-to-first-entry
    exposure."""
    s0 = buf[:, 1].astype(np.int64)
    s1 = buf[:, 5].astype(np.int64)
    t_lo, t_hi = s0.min(), s1.max()
    span = float(t_hi - t_lo)
    lead, mid, tail, occ = [], [], [], np.zeros(5)
    for u in np.unique(sid):
        m = sid == u
        ev = sorted([(int(t), 1) for t in s0[m]] + [(int(t), -1) for t in s1[m]])
        a, b = int(s0[m].min()), int(s1[m].max())
        n, prev, short_mid = 0, a, 0
        occ[0] += (a - t_lo) + (t_hi - b)
        for t, d in ev:
            occ[min(n, 4)] += t - prev
            if n < 4:
                short_mid += (t - prev) * (4 - n) / 4.0  # wave slots empty, as a share of the SIMD's 4
            n, prev = n + d, t
        lead.append(a - t_lo)
        tail.append(t_hi - b)
        mid.append(short_mid)
    ns = len(lead)
    lead, mid, tail = np.array(lead, float), np.array(mid, float), np.array(tail, float)
    print(f"  attribution over {ns} SIMDs, launch span {span / 100:.1f} us (10-ns ticks):")
    print("    SIMD time by resident waves: " + "  ".join(f"{k}:{100 * occ[k] / (ns * span):5.2f} %" for k in range(5)))
    print(f"    fewer than 4 resident: {100 * occ[:4].sum() / (ns * span):.2f} % of SIMD time "
          f"(mean {occ[:4].sum() / ns / 100:.1f} us per SIMD)")
    for name, x in (("lead-in before the SIMD's first wave", lead), ("tail after its last wave", tail),
                    ("empty slots between (slot-weighted)", mid)):
        print(f"    {name:38s} mean {x.mean() / 100:6.2f} us  p90 {np.percentile(x, 90) / 100:6.2f}  max "
              f"{x.max() / 100:6.2f}  ({100 * x.mean() / span:5.2f} % of the span)")
    b = buf.astype(np.float64)
    hash_ = b[:, 2] - b[:, 0]
    first = (buf[:, 3] >> np.uint64(32)).astype(np.float64)
    life = b[:, 4] - b[:, 0]
    to_entry = hash_ + first
    per_simd_waves = len(buf) / ns
    for name, x in (("start -> indices recoded (hash phase)", hash_), ("first gather vmcnt wait", first),
                    ("start -> first entry in registers", to_entry)):
        us = x / (clk * 1e3)
        print(f"    {name:38s} mean {x.mean():8.0f} cyc = {us.mean():6.2f} us  p90 {np.percentile(us, 90):6.2f} us  "
              f"({100 * x.mean() / life.mean():5.2f} % of a wave's lifetime; x {per_simd_waves:.0f} waves per SIMD / 4 "
              f"slots = {100 * us.mean() * per_simd_waves / 4 / (span / 100):5.2f} % of the span)")
    # waves of a SIMD that start within 2 us of another wave of the same SIMD: their front ends coincide
    co = 0
    for u in np.unique(sid):
        t = np.sort(s0[sid == u])
        d = np.diff(t)
        near = np.zeros(len(t), bool)
        near[1:] |= d < 200
        near[:-1] |= d < 200
        co += int(near.sum())
    print(f"    waves starting within 2 us of another wave of their SIMD: {co} of {len(buf)} "
          f"({100 * co / len(buf):.1f} %)")


if __name__ == "__main__":
    main()
