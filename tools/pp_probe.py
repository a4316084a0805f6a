#!/usr/bin/env python3
"""What the primary's PrePrepares cost pbft_replica_push_streams, and what the PrePrepare heads save.

The config-#4 round (n = 256 signers, 2,048 seqs, a Prepare and a Commit of every signer per seq: 2^20 votes) as 256
connection streams, once votes only and once with its 2,048 signed PrePrepares on the primary's connection in front
of the primary's votes.  Every operation is ~100 bytes of text and the votes carry its digest, so with the PrePrepares
every window commits.  The call is timed on a fresh replica per repeat with the heads on
(pbft_replica_set_streams_pp 1: the residue's PrePrepares parsed and hashed by two kernels behind the chain) and off
(every PrePrepare through the general parser, twice, and a blocking one-item pbft_digest_blake2b512 each); the off
legs run twice per repeat, and the distance of their two medians is the spread the goals are judged against.
Counters and events of every leg are checked against the host sequence (push_frames per segment) before anything is
timed.  HIP events time the kernel pair of pbft_wire_decode_preprepares_device over the round's residue.
Copied into a built checkout of the parent commit, whose library lacks the switch, it runs the off legs only.
usage: python tools/pp_probe.py [--reps 20] [--log2n 20] [--op-bytes 100] [--out FILE.json]"""
import argparse
import ctypes
import hashlib
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
    from pbft_amd import GpuBatchVerifier, wire
    from test_replica_streams import SAME, Event, SegHead as CSegHead, Stats, StreamsStats, bind
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--op-bytes", type=int, default=100)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    n_sig = bench.N_REPLICAS
    n = 1 << a.log2n
    n_seq = n // (2 * n_sig)
    n_env = 2 * n_seq
    view, prim = 1, 1 % n_sig
    ops = [(b"transfer %d credits from account %d to account %d; memo: " % (7 * q, q, q + 1)).ljust(a.op_bytes, b".")
           for q in range(1, n_seq + 1)]
    digs = [hashlib.blake2b(op, digest_size=64).digest() for op in ops]
    # the round's envelopes in round order, as bench.envelopes lays them out, over these digests
    base = np.zeros((n_seq, 3, bench.ENVELOPE), np.uint8)
    for s in range(n_seq):
        for kind in (0, 1, 2):
            base[s, kind] = np.frombuffer(b"PBFT" + bytes([kind]) + view.to_bytes(8, "little") +
                                          (s + 1).to_bytes(8, "little") + digs[s], np.uint8)
    msg = np.repeat(base[:, 1:, None, :], n_sig, axis=2).reshape(-1, bench.ENVELOPE)
    key_idx = np.tile(np.arange(n_sig, dtype=np.uint16), n_seq * 2)
    v = GpuBatchVerifier(0)
    seeds = bench.key_seeds(n_sig)
    R, S_good, pub = v.sign(seeds, key_idx, msg, bench.ENVELOPE)
    Sg, bad = bench.corrupt(S_good, bench.ADV_FRAC, bench.SEED)
    Rp, Sp, _ = v.sign(seeds, np.full(n_seq, prim, np.uint16), base[:, 0].copy(), bench.ENVELOPE)
    assert v.set_keys(pub).all()
    lib = bind(v._lib)
    has_switch = hasattr(lib, "pbft_replica_set_streams_pp")
    order = np.argsort(key_idx, kind="stable")  # one connection per signer: its votes in round order
    votes = wire.encode_votes(msg[order, 4].copy(), msg[order, 5:13].copy().view(np.uint64).reshape(n),
                              msg[order, 13:21].copy().view(np.uint64).reshape(n), msg[order, 21:],
                              key_idx[order].astype(np.uint32), np.concatenate([R, Sg], axis=1)[order])
    off, flen, used = wire.frame_index(votes)
    assert len(off) == n and used == len(votes)
    first = np.arange(n_sig + 1, dtype=np.int64) * (n // n_sig)
    start = np.concatenate([off - 2, [len(votes)]]).astype(np.uint64)[first]  # (two-byte varints)
    pps = b"".join(wire.encode_frame(wire.WireMsg(kind=0, view=view, seq=s + 1, digest=digs[s], replica=prim,
                                                  sig=Rp[s].tobytes() + Sp[s].tobytes(), operation=ops[s],
                                                  timestamp=1700000000 + s, client="10.0.0.%d:4%03d" % (s % 250, s % 1000)))
                   for s in range(n_seq))
    cut = int(start[prim])
    with_pp = np.concatenate([votes[:cut], np.frombuffer(pps, np.uint8), votes[cut:]])
    seg_peer = np.arange(n_sig, dtype=np.uint16)

    def segments(extra):
        o = start[:-1].copy()
        ln = (start[1:] - start[:-1]).copy()
        o[prim + 1:] += np.uint64(extra)
        ln[prim] += np.uint64(extra)
        return o, ln
    inputs = {"votes": (torch.from_numpy(votes.copy()).pin_memory().numpy(),) + segments(0),
              "with_pp": (torch.from_numpy(with_pp).pin_memory().numpy(),) + segments(len(pps))}
    out = {"n_votes": n, "n_signers": n_sig, "pre_prepares": n_seq, "op_bytes": a.op_bytes, "reps": a.reps,
           "forged": int(len(bad)), "stream_bytes": {k: int(len(x[0])) for k, x in inputs.items()},
           "library": os.environ.get("PBFT_VERIFY_LIB", "in-tree"), "has_switch": has_switch}

    from replica_sim import lib as replica_lib
    replica_lib()
    keys = pub.tobytes()
    if has_switch:
        lib.pbft_replica_set_streams_pp.argtypes = [ctypes.c_void_p, ctypes.c_int]
        lib.pbft_replica_get_pp_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]

    def replica(on):
        r = ctypes.c_void_p()
        assert lib.pbft_replica_create(v._ctx, n_sig, 0, keys, ctypes.byref(r)) == 0
        assert lib.pbft_replica_reserve_streams(r, len(with_pp), n_sig, n + n_seq, n_env, 4096) == 0
        if has_switch:
            assert lib.pbft_replica_set_streams_pp(r, on) == 0
        return r

    def counters(r):
        s = Stats()
        lib.pbft_replica_get_stats(r, ctypes.byref(s))
        return {k: getattr(s, k) for k in SAME}

    ev, ne = (Event * 16384)(), ctypes.c_uint32()
    heads = (CSegHead * n_sig)()

    def host_sequence(r, which):
        stream, so, sl = inputs[which]
        used, x, y = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        assert lib.pbft_replica_flush(r, 1, ev, 16384, ctypes.byref(ne)) == 0
        events = [(e.view, e.seq, e.kind) for e in ev[:ne.value]]
        for s in range(n_sig):
            buf = (ctypes.c_char * int(sl[s])).from_buffer(stream, int(so[s]))
            assert lib.pbft_replica_push_frames(r, s, buf, int(sl[s]), ctypes.byref(used), ctypes.byref(x),
                                                ctypes.byref(y)) == 0 and used.value == sl[s]
        assert lib.pbft_replica_flush(r, 1, ev, 16384, ctypes.byref(ne)) == 0
        return sorted(events + [(e.view, e.seq, e.kind) for e in ev[:ne.value]])

    def call(r, which):
        stream, so, sl = inputs[which]
        x, y = ctypes.c_uint64(), ctypes.c_uint64()
        rc = lib.pbft_replica_push_streams(r, stream.ctypes.data, len(stream), so.ctypes.data, sl.ctypes.data,
                                           seg_peer.ctypes.data, n_sig, heads, ctypes.byref(x), ctypes.byref(y), ev,
                                           16384, ctypes.byref(ne))
        assert rc == 0 and x.value == n + (n_seq if which == "with_pp" else 0), (rc, x.value, y.value)
        return [(e.view, e.seq, e.kind) for e in ev[:ne.value]]

    # 1. outputs first: every leg against the host sequence on the same bytes (a context serves one replica at a time)
    ss = StreamsStats()
    for which in ("votes", "with_pp"):
        r = replica(0)
        want_ev = host_sequence(r, which)
        want = counters(r)
        lib.pbft_replica_destroy(r)
        assert want["rejected_sig"] == len(bad)
        out.setdefault("events", {})[which] = len(want_ev)
        for on in ((1, 0) if has_switch else (0,)):
            r = replica(on)
            got_ev = call(r, which)
            assert got_ev == want_ev and counters(r) == want, (which, on)
            lib.pbft_replica_get_streams_stats(r, ctypes.byref(ss))
            assert ss.calls_device == 1 and ss.clean_rows == n and ss.residue_rows == (n_seq if which == "with_pp" else 0)
            if has_switch:
                pst = (ctypes.c_uint64 * 2)()
                assert lib.pbft_replica_get_pp_stats(r, pst) == 0
                assert tuple(pst) == (((n_seq, 0) if on else (0, n_seq)) if which == "with_pp" else (0, 0)), tuple(pst)
            lib.pbft_replica_destroy(r)
    out["checked"] = "events and counters of every leg equal the host sequence's"

    # 2. the call, interleaved, a fresh replica each
    legs = [("votes_off", "votes", 0), ("votes_off_again", "votes", 0), ("with_pp_off", "with_pp", 0),
            ("with_pp_off_again", "with_pp", 0)]
    if has_switch:
        legs += [("votes_on", "votes", 1), ("with_pp_on", "with_pp", 1)]
    t = {name: [] for name, _, _ in legs}
    front = {name: [] for name, _, _ in legs}
    for _ in range(a.reps):
        for name, which, on in legs:
            r = replica(on)
            t0 = time.perf_counter()
            call(r, which)
            t[name].append((time.perf_counter() - t0) * 1e3)
            lib.pbft_replica_get_streams_stats(r, ctypes.byref(ss))
            front[name].append(ss.front_ns * 1e-6)
            lib.pbft_replica_destroy(r)
    res = {"push_streams_ms": {k: stats(x) for k, x in t.items()}, "front_ms": {k: stats(x) for k, x in front.items()}}
    m = {k: res["push_streams_ms"][k]["median"] for k in t}
    spread = max(abs(m["votes_off"] - m["votes_off_again"]), abs(m["with_pp_off"] - m["with_pp_off_again"]))
    res["spread_off_vs_off_ms"] = spread
    res["pre_prepares_cost_off_ms"] = m["with_pp_off"] - m["votes_off"]
    if has_switch:
        res["pre_prepares_cost_on_ms"] = m["with_pp_on"] - m["votes_on"]
        saved = res["pre_prepares_cost_off_ms"] - res["pre_prepares_cost_on_ms"]
        res["goal_pre_prepares_cheaper_with_heads"] = {"saved_ms": saved, "met": bool(saved > spread)}
        slower = m["votes_on"] - m["votes_off"]
        res["goal_votes_only_not_slower"] = {"on_minus_off_ms": slower, "met": bool(slower <= spread)}
    res["note"] = ("wall clock of the blocking call on one host thread, a fresh replica per call (creation not timed); "
                   "front = the GPU chain with its copies, the PrePrepare kernels included")
    out["host"] = res

    # 3. the kernel pair over the round's residue, HIP events on the launch stream
    if has_switch:
        from pbft_amd.wire import AdmitResidue, PpHead
        stream = inputs["with_pp"][0]
        res_np = np.zeros(n_seq, AdmitResidue)
        o, fl, _ = wire.frame_index(stream[cut:cut + len(pps)])
        res_np["off"], res_np["frame"], res_np["len"] = o + np.uint64(cut), np.arange(n_seq), fl
        dev = torch.device("cuda", 0)
        d_stream = torch.from_numpy(np.concatenate([stream, np.zeros((-len(stream)) % 16, np.uint8)])).to(dev)
        d_res = torch.from_numpy(res_np.view(np.uint8)).to(dev)
        d_pp = torch.zeros(n_seq * PpHead.itemsize, dtype=torch.uint8, device=dev)
        st = torch.cuda.Stream(dev)
        ms = []
        for rep in range(a.reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                e0.record(st)
                assert lib.pbft_wire_decode_preprepares_device(v._ctx, d_stream.data_ptr(), len(stream), d_res.data_ptr(),
                                                               None, n_seq, d_pp.data_ptr(), st.cuda_stream) == 0
                e1.record(st)
            torch.cuda.synchronize()
            if rep >= 2:
                ms.append(e0.elapsed_time(e1))
        got = d_pp.cpu().numpy().view(PpHead)
        assert (got["status"] == wire.PP_OK).all() and got["computed"].tobytes() == b"".join(digs)
        out["device"] = {"pp_parse_and_digest_kernels_ms": stats(ms), "entries": n_seq,
                         "note": "HIP events around pp_parse_kernel + pp_digest_kernel, one launch pair"}
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    v.close()


if __name__ == "__main__":
    main()
