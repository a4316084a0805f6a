"""Generate tests/golden/comb_edges.npz: valid signatures whose comb digits sit on the table edges.

CPU only, run offline (python tests/golden/gen_comb_edges.py [workers]); needs oracle/liboracle.so (make -C oracle).

One key (seed SEED, clamped scalar a, A = [a]B) and one nonce r (R = [r]B) are fixed.  For every candidate envelope
M, k = SHA-512(R || A || M) mod L and s = (r + k a) mod L make (R, s) a valid signature of M under A -- verification
does not care that r is not the RFC 8032 nonce -- at the cost of one hash and one multiply mod L.  s is recoded under
the base-point plan and k under the four key plans (tests/comb_edges.py); the first envelope found for each (plan,
position, target) is kept, and the search ends only when every target of every plan is present.  Each kept row is
followed by a twin whose s differs by one unit of the tagged position (and is still below L), which must be rejected.

A second search over the same envelopes keeps those whose RFC 8032 nonce SHA-512(prefix || M) mod L has base-table
digit 0 or -2^(w-1) at a position (0 at the top): the inputs of the signing kernels.

Expected bits come from oracle/ed25519_ref.py verify_strict and are checked against the C oracle.

Columns: key [32], seed [32], R / S [n][32], msg [n][85], expected, twin [n] u8, plan (0 = base table, digits of s;
13 / 14 / 16 / 32 = that key plan, digits of k), pos, target [n]; sg_seed, sg_pub [32], sg_msg [m][85], sg_pos,
sg_target [m], sg_R / sg_S [m][32] (ed25519_ref.sign).
"""
import ctypes
import hashlib
import multiprocessing as mp
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import comb_edges as ce  # noqa: E402
import ed25519_ref as ref  # noqa: E402

L = ce.L
SEED = hashlib.sha512(b"pbft-comb-edges-key").digest()[:32]
NONCE = int.from_bytes(hashlib.sha512(b"pbft-comb-edges-nonce").digest(), "little") % L
DIGEST = hashlib.blake2b(b"comb-edges", digest_size=64).digest()
CHUNK = 1 << 18        # tries per work item
KEY_CHUNKS = 64        # the key plans' windows are at most 20 bits wide: 2^24 tries hold all their targets
SEQ_BITS = 24          # try t is the envelope of view t >> 24, seq t & (2^24 - 1), kind 1 + (view & 1)


def try_envelope(t):
    view = t >> SEQ_BITS
    return ce.envelope(1 + (view & 1), view, t & ((1 << SEQ_BITS) - 1), DIGEST)


def recode_const(plan):
    """C with: window i of x + C is digit i of x plus 2^(w_i - 1), for every position but the top (whose window of
    x + C is its digit) -- the carries of `digits::take` are the carries of this one addition."""
    return sum(1 << (ce.bitoff(plan, pos) + ce.width(plan, pos) - 1) for pos in range(plan[0] - 1))


def windows(buf, plan, n):
    """The windows of n 32-byte little-endian numbers, one uint64 array per position."""
    a = np.frombuffer(buf, dtype="<u8").reshape(n, 4)
    out = []
    for pos in range(plan[0]):
        o, w = ce.bitoff(plan, pos), ce.width(plan, pos)
        q, sh = divmod(o, 64)
        v = a[:, q] >> np.uint64(sh)
        if sh + w > 64:
            v = v | (a[:, q + 1] << np.uint64(64 - sh))
        out.append(v & np.uint64((1 << w) - 1))
    return out


def scan_chunk(args):
    """Tries [c * CHUNK, (c + 1) * CHUNK): ([(plan id, pos, target, try)] first hits in this chunk, same for the
    signer set with plan id -1)."""
    c, want_base, want_key, want_signer = args
    a, prefix = ref.secret_expand(SEED)
    Ab = ref.public_key(SEED)
    Rb = ref.compress(ref.pt_mul(NONCE, ref.BASE))
    cb = recode_const(ce.PLAN_B)
    kc = {pid: recode_const(pl) for pid, pl in ce.KEY_PLANS.items()}
    t0 = c * CHUNK
    assert CHUNK <= 1 << SEQ_BITS and (t0 >> SEQ_BITS) == ((t0 + CHUNK - 1) >> SEQ_BITS)
    head = try_envelope(t0)[:13]                                  # "PBFT", kind, view: constant over the chunk
    hv, hs = hashlib.sha512(Rb + Ab + head), hashlib.sha512(prefix + head)
    seq0 = t0 & ((1 << SEQ_BITS) - 1)
    sbuf, nbuf, kbuf = [], [], {pid: [] for pid in kc}
    frm, r = int.from_bytes, NONCE
    for i in range(seq0, seq0 + CHUNK):
        tail = i.to_bytes(8, "little") + DIGEST
        if want_base or want_key:
            h = hv.copy()
            h.update(tail)
            k = frm(h.digest(), "little") % L
            sbuf.append(((r + k * a) % L + cb).to_bytes(32, "little"))
            if want_key:
                for pid, cst in kc.items():
                    kbuf[pid].append((k + cst).to_bytes(32, "little"))
        if want_signer:
            h = hs.copy()
            h.update(tail)
            nbuf.append((frm(h.digest(), "little") % L + cb).to_bytes(32, "little"))
    hits, shits = [], []

    def first_hits(buf, pid, plan, tgts, out):
        for pos, u in enumerate(windows(b"".join(buf), plan, CHUNK)):
            top = pos == plan[0] - 1
            half = 1 << (ce.width(plan, pos) - 1)
            for tg in tgts(pos):
                idx = np.flatnonzero(u == np.uint64(tg if top else tg + half))
                if len(idx):
                    out.append((pid, pos, tg, t0 + int(idx[0])))

    if want_base:
        first_hits(sbuf, 0, ce.PLAN_B, lambda pos: ce.targets(ce.PLAN_B, pos), hits)
    if want_key:
        for pid, plan in ce.KEY_PLANS.items():
            first_hits(kbuf[pid], pid, plan, lambda pos, plan=plan: ce.targets(plan, pos), hits)
    if want_signer:
        first_hits(nbuf, -1, ce.PLAN_B, ce.signer_targets, shits)
    return c, hits, shits


def search(workers):
    want = {tg for pid in ce.PLANS for tg in ce.all_targets(pid)}
    swant = {(-1, pos, tg) for pos in range(ce.PLAN_B[0]) for tg in ce.signer_targets(pos)}
    assert len(swant) == ce.SIGNER_COUNT
    found, sfound = {}, {}
    base_left = lambda: any(t[0] == 0 and t not in found for t in want)  # noqa: E731
    pending, nxt, done = {}, 0, 0
    with mp.Pool(workers) as pool:
        while len(found) < len(want) or len(sfound) < len(swant):
            while len(pending) < 2 * workers:
                pending[nxt] = pool.apply_async(scan_chunk, ((nxt, base_left(), nxt < KEY_CHUNKS,
                                                              len(sfound) < len(swant)),))
                nxt += 1
            c, hits, shits = pending.pop(done).get()   # in chunk order: the first try found for a target is kept
            done += 1
            for pid, pos, tg, t in hits:
                found.setdefault((pid, pos, tg), t)
            for pid, pos, tg, t in shits:
                sfound.setdefault((pid, pos, tg), t)
            if done % 64 == 0:
                print(f"  {done * CHUNK / 1e6:.0f} M tries: {len(found)}/{len(want)} verifier targets, "
                      f"{len(sfound)}/{len(swant)} signer targets", flush=True)
            assert done < KEY_CHUNKS or all(t in found for t in want if t[0] != 0), "key-plan targets missing"
        pool.terminate()
    assert set(found) == want and set(sfound) == swant
    return found, sfound, done * CHUNK


def oracle_bits(key, R, S, msg):
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))
    vp = ctypes.c_void_p
    lib.oracle_verify_batch.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32,
                                        ctypes.c_uint64, vp, ctypes.c_int]
    n = len(R)
    keys = np.ascontiguousarray(key.reshape(1, 32))
    kidx, out = np.zeros(n, np.uint16), np.zeros(n, np.uint8)
    buf = np.zeros(n * 85 + 16, np.uint8)
    buf[: n * 85] = msg.reshape(-1)
    assert lib.oracle_verify_batch(keys.ctypes.data, 1, R.ctypes.data, S.ctypes.data, kidx.ctypes.data,
                                   buf.ctypes.data, 85, 85, n, out.ctypes.data, 4) == 0
    return out.astype(bool)


def twin_scalar(s, plan, pos, d):
    """s with one unit of position pos added or taken away, so that the position's digit moves by one without
    leaving its range, and the twin stays in [0, L)."""
    unit = 1 << ce.bitoff(plan, pos)
    top = pos == plan[0] - 1
    step = -unit if (d == (1 << (ce.width(plan, pos) - 1)) - 1 and not top) else unit
    s2 = s + step
    if not 0 <= s2 < L:
        s2 = s - step
    assert 0 <= s2 < L and s2 != s
    return s2


def main():
    workers = int(sys.argv[1]) if len(sys.argv) > 1 else (os.cpu_count() or 1)
    t_start = time.time()
    found, sfound, tries = search(workers)
    t_search = time.time() - t_start
    a, _ = ref.secret_expand(SEED)
    Ab = ref.public_key(SEED)
    Rb = ref.compress(ref.pt_mul(NONCE, ref.BASE))
    cols = {k: [] for k in ("R", "S", "msg", "expected", "twin", "plan", "pos", "target")}
    for (pid, pos, tg), t in sorted(found.items()):
        M = try_envelope(t)
        k = int.from_bytes(hashlib.sha512(Rb + Ab + M).digest(), "little") % L
        s = (NONCE + k * a) % L
        plan = ce.PLANS[pid]
        assert ce.recode(s if pid == 0 else k, plan)[pos] == tg
        s2 = twin_scalar(s, plan, pos, tg)
        if pid == 0:
            assert abs(ce.recode(s2, plan)[pos] - tg) == 1
        for sv, tw in ((s, 0), (s2, 1)):
            sb = sv.to_bytes(32, "little")
            bit = ref.verify_strict(Ab, Rb + sb, M)
            assert bit == (not tw)
            for name, v in (("R", Rb), ("S", sb), ("msg", M)):
                cols[name].append(np.frombuffer(v, np.uint8))
            for name, v in (("expected", bit), ("twin", tw), ("plan", pid), ("pos", pos), ("target", tg)):
                cols[name].append(v)
    out = {"key": np.frombuffer(Ab, np.uint8), "seed": np.frombuffer(SEED, np.uint8),
           "R": np.stack(cols["R"]), "S": np.stack(cols["S"]), "msg": np.stack(cols["msg"]),
           "expected": np.array(cols["expected"], np.uint8), "twin": np.array(cols["twin"], np.uint8),
           "plan": np.array(cols["plan"], np.int16), "pos": np.array(cols["pos"], np.int16),
           "target": np.array(cols["target"], np.int32)}
    assert (oracle_bits(out["key"], out["R"], out["S"], out["msg"]) == out["expected"].astype(bool)).all()
    for pid, cnt in ce.COUNTS.items():
        assert int(((out["plan"] == pid) & (out["twin"] == 0)).sum()) == cnt
    assert len(out["S"]) % 64
    sg = sorted(sfound.items())
    _, prefix = ref.secret_expand(SEED)
    for (_, pos, tg), t in sg:
        rn = int.from_bytes(hashlib.sha512(prefix + try_envelope(t)).digest(), "little") % L
        assert ce.recode(rn, ce.PLAN_B)[pos] == tg
    sigs = [ref.sign(SEED, try_envelope(t)) for _, t in sg]
    out.update({"sg_seed": out["seed"], "sg_pub": out["key"],
                "sg_msg": np.stack([np.frombuffer(try_envelope(t), np.uint8) for _, t in sg]),
                "sg_pos": np.array([k[1] for k, _ in sg], np.int16),
                "sg_target": np.array([k[2] for k, _ in sg], np.int32),
                "sg_R": np.stack([np.frombuffer(x[:32], np.uint8) for x in sigs]),
                "sg_S": np.stack([np.frombuffer(x[32:], np.uint8) for x in sigs])})
    assert len(sg) == ce.SIGNER_COUNT
    np.savez_compressed(ce.FIXTURE, **out)
    print(f"{len(out['S'])} rows + {len(sg)} signer envelopes, {tries / 1e6:.0f} M tries, search {t_search:.0f} s "
          f"with {workers} workers, {os.path.getsize(ce.FIXTURE)} bytes")


if __name__ == "__main__":
    main()
