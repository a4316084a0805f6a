"""The frame index made on the GPU (pbft_wire_index_streams_device, pbft_verify_streams_tally_device,
pbft_verify_streams_tally): per-connection segments of one stream, at unaligned offsets with gaps between them, against
the host walk pbft_wire_frame_index called per segment through ctypes -- never against the code under test.  Every
device output has 256 poisoned guard bytes behind it; the gaps and the tail of the stream are filled with 0x7B and 0x00
bytes, both of which look like the start of a frame."""
import ctypes

import numpy as np
import pytest

from test_gpu_frames import GUARD, dev_bytes
from test_gpu_frames_tally import Case, TallyOut
from test_gpu_verify import gv  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
TILES = (512, 2048, 0)  # 0: the default
UVI_MAX = 1 << 27


# ---- streams ----
def uvi(v):
    from pbft_amd import wire
    return wire.uvi_encode(v)


def frame(rng, n):
    """A frame of n body bytes that look like headers: small values, continuation bytes, zeroes."""
    mode = int(rng.integers(3))
    if mode == 0:
        body = rng.integers(0, 256, n, dtype=np.uint8)
    elif mode == 1:
        body = rng.choice(np.array([0x00, 0x01, 0x7B, 0x80, 0xFF, 0x81, 0x02, 0xD4], np.uint8), n)
    else:
        body = np.full(n, 0x80, np.uint8)
    return uvi(n) + body.tobytes()


def votes(rng, n):
    return b"".join(frame(rng, int(rng.integers(336, 380))) for _ in range(n))


def lay_out(rng, parts, outside=()):
    """The segments `parts` (bytes each) at unaligned offsets with poisoned gaps between them and behind the last.
    Segments named in `outside` are not laid out: they claim bytes that end behind the stream.
    Returns (stream uint8, seg_off, seg_len)."""
    chunks, off, at = [], [], 0
    for s, p in enumerate(parts):
        gap = int(rng.integers(1, 40))
        chunks.append(rng.choice(np.array([0x7B, 0x00], np.uint8), gap).tobytes())
        at += gap
        off.append(at)
        if s not in outside:
            chunks.append(p)
            at += len(p)
    tail = int(rng.integers(1, 30))
    chunks.append(rng.choice(np.array([0x7B, 0x00], np.uint8), tail).tobytes())
    stream = np.frombuffer(b"".join(chunks), np.uint8)
    for s in outside:
        off[s] = len(stream) - len(parts[s]) + 1 + s % 3
    return stream, np.array(off, np.uint64), np.array([len(p) for p in parts], np.uint64)


def split(data_frames, bounds):
    """Consecutive runs of whole frames: data_frames[bounds[i] : bounds[i + 1]] joined."""
    return [b"".join(data_frames[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]


# ---- the oracle ----
def oracle(stream, seg_off, seg_len, seg_peer, frame_cap):
    """pbft_wire_frame_index per segment: (off, len, peer) padded to frame_cap, seg heads, (total, not written)."""
    import pbft_amd
    lib = pbft_amd.load()
    off, flen, peer = [], [], []
    heads = np.zeros(len(seg_off), pbft_amd.SegHead)
    run = 0
    for s, (o, ln) in enumerate(zip(seg_off.tolist(), seg_len.tolist())):
        heads[s]["first"] = len(off)
        inside = o + ln <= len(stream)
        if inside:
            run += ln
            inside = run <= len(stream)
        if not inside:
            heads[s]["status"] = 2
            continue
        seg = np.ascontiguousarray(stream[o:o + ln])
        o_, l_ = np.zeros(ln + 1, np.uint64), np.zeros(ln + 1, np.uint32)
        n, used = ctypes.c_uint64(), ctypes.c_uint64()
        rc = lib.pbft_wire_frame_index(seg.ctypes.data if ln else None, ln, ln + 1, o_.ctypes.data, l_.ctypes.data,
                                       ctypes.byref(n), ctypes.byref(used))
        assert rc in (0, -1)
        heads[s]["status"], heads[s]["n_frames"], heads[s]["consumed"] = (1 if rc else 0), n.value, used.value
        off += (o_[:n.value] + np.uint64(o)).tolist()
        flen += l_[:n.value].tolist()
        peer += [int(seg_peer[s]) if seg_peer is not None else 0] * n.value
    total = len(off)
    pad = max(0, frame_cap - total)
    res = dict(off=np.array(off[:frame_cap] + [0] * pad, np.uint64), len=np.array(flen[:frame_cap] + [0] * pad, np.uint32),
               peer=np.array(peer[:frame_cap] + [0xFFFF] * pad, np.uint16), heads=heads, total=total,
               n_frames=np.array([total, max(0, total - frame_cap)], np.uint32))
    return res


class DevIndex:
    """A stream and its segment table on the device, poisoned index outputs with guards behind them."""
    FILL = dict(off=0xA5, len=0x5A, peer=0xC3, heads=0x3C, nfr=0x96)

    def __init__(self, stream, seg_off, seg_len, seg_peer, frame_cap):
        import torch
        self.nbytes, self.S, self.cap = len(stream), len(seg_off), frame_cap
        self.s = dev_bytes(stream, pad=(-len(stream)) % 16)  # readable up to the next multiple of 16, no further
        self.so, self.sl = dev_bytes(seg_off.astype(np.uint64)), dev_bytes(seg_len.astype(np.uint64))
        self.sp = dev_bytes(seg_peer.astype(np.uint16)) if seg_peer is not None else None
        self.size = dict(off=8 * frame_cap, len=4 * frame_cap, peer=2 * frame_cap, heads=24 * self.S, nfr=8)
        dev = torch.device("cuda", 0)
        self.t = {k: torch.full((n + GUARD,), self.FILL[k], dtype=torch.uint8, device=dev) for k, n in self.size.items()}

    def args(self):
        p = self.sp is not None
        return dict(d_stream=self.s.data_ptr(), stream_bytes=self.nbytes, d_seg_off=self.so.data_ptr() if self.S else 0,
                    d_seg_len=self.sl.data_ptr() if self.S else 0, n_segments=self.S, frame_cap=self.cap,
                    d_off=self.t["off"].data_ptr(), d_len=self.t["len"].data_ptr(),
                    d_seg_heads=self.t["heads"].data_ptr(), d_n_frames=self.t["nfr"].data_ptr(),
                    d_seg_peer=self.sp.data_ptr() if p and self.S else 0, d_peer=self.t["peer"].data_ptr() if p else 0)

    def poison(self):
        for k, t in self.t.items():
            t.fill_(self.FILL[k])

    def untouched(self):
        return all((t.cpu().numpy() == self.FILL[k]).all() for k, t in self.t.items())

    def read(self):
        import pbft_amd
        r = {k: t.cpu().numpy() for k, t in self.t.items()}
        for k, a in r.items():
            assert (a[self.size[k]:] == self.FILL[k]).all(), ("guard overwritten", k)
        cut = {k: a[:self.size[k]].copy() for k, a in r.items()}
        return dict(off=cut["off"].view(np.uint64), len=cut["len"].view(np.uint32), peer=cut["peer"].view(np.uint16),
                    heads=cut["heads"].view(pbft_amd.SegHead), n_frames=cut["nfr"].view(np.uint32))


def check_index(got, exp, where, peers=True):
    assert got["n_frames"].tolist() == exp["n_frames"].tolist(), (where, got["n_frames"], exp["n_frames"])
    for k in ("status", "n_frames", "consumed", "first", "pad"):
        bad = np.nonzero(got["heads"][k] != exp["heads"][k])[0]
        assert len(bad) == 0, (where, k, bad[:8], got["heads"][bad[:8]], exp["heads"][bad[:8]])
    for k in ("off", "len") + (("peer",) if peers else ()):
        bad = np.nonzero(got[k] != exp[k])[0]
        assert len(bad) == 0, (where, k, bad[:8], got[k][bad[:8]], exp[k][bad[:8]])


def run_index(gv, stream, seg_off, seg_len, seg_peer, frame_cap, tiles=TILES, where=""):
    """The index at every tile size against the oracle; returns the oracle's result."""
    import torch
    exp = oracle(stream, seg_off, seg_len, seg_peer, frame_cap)
    d = DevIndex(stream, seg_off, seg_len, seg_peer, frame_cap)
    ts = torch.cuda.Stream()
    try:
        for tile in tiles:
            gv.set_option(gv.OPT_INDEX_TILE, tile)
            d.poison()
            torch.cuda.synchronize()
            gv.index_streams_device(stream=ts.cuda_stream, **d.args())
            ts.synchronize()
            check_index(d.read(), exp, (where, tile), peers=seg_peer is not None)
            if seg_peer is None:
                assert (d.t["peer"].cpu().numpy() == d.FILL["peer"]).all()
    finally:
        gv.set_option(gv.OPT_INDEX_TILE, 0)
    return exp


def unequal_bounds(rng, n, parts):
    """parts + 1 increasing bounds over n frames, the runs of very different lengths."""
    if parts == 1:
        return [0, n]
    cuts = np.sort(rng.choice(np.arange(1, n), parts - 1, replace=False))
    return [0] + cuts.tolist() + [n]


# ---- 1. index only ----
@pytest.mark.parametrize("S", [1, 3, 37])
def test_random_bodies(gv, S):
    """~600 frames in S segments of unequal length (S >= 3: one of them empty, one ending behind the stream), ~400
    tiles of 512 bytes: off / len / peer / heads / totals equal the host walk's at tile 512, 2048 and the default."""
    rng = np.random.default_rng(100 + S)
    frames = [frame(rng, int(rng.integers(336, 380)) if rng.random() < 0.9 else int(rng.integers(0, 200)))
              for _ in range(600)]
    real = S if S < 3 else S - 2
    parts = split(frames, unequal_bounds(rng, 600, real))
    outside = ()
    if S >= 3:
        parts.insert(1, b"")
        parts.append(votes(rng, 2))
        outside = (S - 1,)
    assert len(parts) == S
    stream, so, sl = lay_out(rng, parts, outside)
    peer = rng.integers(0, 65535, S).astype(np.uint16)
    exp = run_index(gv, stream, so, sl, peer, 640, where=S)
    assert exp["total"] == 600 and (exp["heads"]["status"] == 2).sum() == len(outside)
    assert len(set((exp["off"][:600] % 16).tolist())) == 16  # bodies start at every offset mod 16
    assert len(stream) > 300 * 512 and (S < 3 or exp["heads"]["n_frames"][1] == 0)
    run_index(gv, stream, so, sl, None, 640, tiles=(512,), where=(S, "no peers"))


@pytest.mark.parametrize("S", [1, 255])
def test_default_tile_3000_frames(gv, S):
    """One 3,000-frame stream as one segment (~63 tiles of 16 KiB) and as 255 segments shorter than a tile."""
    rng = np.random.default_rng(200 + S)
    frames = [frame(rng, int(rng.integers(336, 380))) for _ in range(3000)]
    parts = split(frames, unequal_bounds(rng, 3000, S))
    stream, so, sl = lay_out(rng, parts)
    peer = rng.integers(0, 65535, S).astype(np.uint16)
    exp = run_index(gv, stream, so, sl, peer, 3000, tiles=(0, 512), where=S)
    assert exp["total"] == 3000 and (exp["heads"]["status"] == 0).all()
    assert S == 1 or sl.max() < 16384 * 4 and np.median(sl) < 16384


# ---- 2. hard shapes ----
def test_hard_shapes(gv):
    """A run of 1,000 zero-length frames; lengths 127 / 128 / 16383 / 16384; one 70,000-byte frame between votes (a
    three-byte varint, > 100 tiles of 512 skipped); a PrePrepare-sized frame, so that the next entry is >= 384; a
    two-byte varint that straddles a tile edge; a varint cut by the segment's end."""
    rng = np.random.default_rng(7)
    b = b"".join(frame(rng, 0) for _ in range(1000))
    for n in (127, 128, 16383, 16384):
        b += frame(rng, n) + votes(rng, 2)
    b += frame(rng, 70000) + votes(rng, 3) + frame(rng, 1100) + votes(rng, 3)
    gap = (511 - len(b)) % 512  # the next-but-one header starts on byte 511 of a tile
    if gap < 400:  # (398..909 body bytes: a two-byte varint, and no other frame here has that length)
        gap += 512
    b += frame(rng, gap - 2) + votes(rng, 4)
    whole = len(b)
    b += uvi(300)[:1]  # 0xAC: the first byte of a two-byte varint, cut by the segment's end
    stream, so, sl = lay_out(rng, [votes(rng, 3), b, votes(rng, 2)])
    exp = run_index(gv, stream, so, sl, np.array([1, 2, 3], np.uint16), 1100, where="hard")
    h = exp["heads"][1]
    assert h["status"] == 0 and h["consumed"] == whole and h["n_frames"] == 1000 + 12 + 1 + 3 + 1 + 3 + 1 + 4
    lens = exp["len"][3:3 + h["n_frames"]]
    straddler = np.nonzero(lens == gap - 2)[0][-1] + 1  # the frame behind the filler
    assert (int(exp["off"][3 + straddler]) - 2 - int(so[1])) % 512 == 511
    assert {0, 127, 128, 16383, 16384, 70000, 1100} <= set(lens.tolist())


# ---- 3. errors and stops ----
def tails():
    """(name, bytes, framing error?) of every stop and error class."""
    t = [("0x80 x %d" % k, b"\x80" * k, k >= 10) for k in range(1, 12)]
    t += [("non-minimal", b"\x80\x00", True), ("2^27", uvi(UVI_MAX) + b"\x11" * 9, False),
          ("2^27 + 1", uvi(UVI_MAX + 1) + b"\x11" * 9, True), ("> u64", b"\xff" * 9 + b"\x02", True),
          ("cut body", uvi(350) + b"\x7b" * 200, False), ("cut varint", uvi(300)[:1], False),
          ("cut 3-byte varint", uvi(70000)[:2], False)]
    return t


def test_errors_and_stops(gv):
    """Every error and stop class at the start of its segment, in the middle and with its varint on a tile's last
    byte; an error has whole frames behind it, which are not delivered; clean segments between the failing ones are
    delivered whole."""
    rng = np.random.default_rng(3)
    parts, want = [], []
    for name, t, err in tails():
        for place in ("start", "mid", "edge"):
            if place == "start":
                head, n = b"", 0
            elif place == "mid":
                n = int(rng.integers(2, 7))
                head = votes(rng, n)
            else:
                head = votes(rng, 2)
                gap = (511 - len(head)) % 512
                if gap < 130:
                    gap += 512
                head += frame(rng, gap - 2)
                n = 3
                assert len(head) % 512 == 511
            parts.append(head + t + (votes(rng, 2) if err else b""))
            want.append((name, place, n, len(head), 1 if err else 0))
            parts.append(votes(rng, 3))  # the neighbour
            want.append(("clean", place, 3, len(parts[-1]), 0))
    stream, so, sl = lay_out(rng, parts)
    S = len(parts)
    exp = run_index(gv, stream, so, sl, np.arange(S).astype(np.uint16), 400, tiles=(512, 0), where="errors")
    for s, (name, place, n, consumed, status) in enumerate(want):
        h = exp["heads"][s]
        assert (h["n_frames"], h["consumed"], h["status"]) == (n, consumed, status), (name, place, h)
    assert exp["total"] == sum(w[2] for w in want) <= 400


# ---- 4. frame_cap ----
def test_frame_cap(gv):
    """frame_cap below the total: the first frame_cap entries are exact, d_n_frames[1] holds the rest, the heads are
    complete, the guards intact; frame_cap = 0; frame_cap above the total: padding entries off 0, len 0, peer
    0xFFFF."""
    rng = np.random.default_rng(4)
    frames = [frame(rng, int(rng.integers(336, 380))) for _ in range(300)]
    parts = split(frames, unequal_bounds(rng, 300, 5))
    stream, so, sl = lay_out(rng, parts)
    peer = np.array([9, 8, 7, 6, 5], np.uint16)
    for cap in (263, 1, 0, 300, 301, 1000):
        exp = run_index(gv, stream, so, sl, peer, cap, tiles=(512,), where=cap)
        assert exp["n_frames"].tolist() == [300, max(0, 300 - cap)] and exp["heads"]["n_frames"].sum() == 300
        if cap > 300:
            assert (exp["peer"][300:] == 0xFFFF).all() and not exp["off"][300:].any() and not exp["len"][300:].any()
    # no segment at all: the totals are written, the entries are padding
    exp = run_index(gv, stream, so[:0], sl[:0], peer[:0], 7, tiles=(512,), where="S = 0")
    assert exp["n_frames"].tolist() == [0, 0]


def test_tile_option(gv):
    from pbft_amd import PbftError
    for bad in (500, 256, 1, 32768, 3 * 512):
        with pytest.raises(PbftError) as e:
            gv.set_option(gv.OPT_INDEX_TILE, bad)
        assert e.value.code == -1, bad
    for good in (512, 1024, 16384, 0):
        gv.set_option(gv.OPT_INDEX_TILE, good)


# ---- 5..7. the whole chain ----
@pytest.fixture(scope="module")
def cases(gv):
    return {4: Case(gv, 4, 420, 12), 256: Case(gv, 256, 300, 24)}


def connections(c, S, rng):
    """The frames of Case c dealt to S connections (connection k's peer is k % n_keys; a frame goes to a connection
    of its signer where there is one, so most votes pass the peer rule and the rest are ESIGNER); some connections end
    in a truncated frame, one has a framing error halfway.  Returns (stream, seg_off, seg_len, seg_peer)."""
    start = np.concatenate([[0], (c.off + c.flen)[:-1]]).astype(np.int64)
    end = (c.off + c.flen).astype(np.int64)
    raw = c.stream.tobytes()
    seg_peer = (np.arange(S) % c.n_keys).astype(np.uint16)
    conns = [[] for _ in range(S)]
    for f in range(c.n):
        key = int(c.heads["key_idx"][f])
        mine = [k for k in range(S) if seg_peer[k] == key]
        k = mine[f % len(mine)] if mine else f % S
        conns[k].append(raw[start[f]:end[f]])
    parts = []
    broken = max(range(S), key=lambda k: len(conns[k]))
    for k, fr in enumerate(conns):
        p = b"".join(fr)
        if k == broken:  # a non-minimal varint halfway: the frames behind it are lost
            half = len(fr) // 2
            p = b"".join(fr[:half]) + b"\x80\x00" + b"".join(fr[half:])
        elif k % 3 == 1 and fr and len(fr[0]) > 1:  # a last frame still on its way
            p += fr[0][:int(rng.integers(1, len(fr[0])))]
        parts.append(p)
    stream, so, sl = lay_out(rng, parts)
    return stream, so, sl, seg_peer


@pytest.mark.parametrize("n_keys,S", [(4, 3), (4, 37), (256, 3), (256, 37)])
def test_verify_streams_tally(gv, cases, n_keys, S):
    """Every output is word for word that of verify_frames_tally given the host index of every segment and per-frame
    peers, with truncated last frames, a framing error halfway through one connection, and connections whose peer is
    not their frames' replica."""
    from pbft_amd import bitmap_to_bool
    c = cases[n_keys]
    assert gv.set_keys(c.pub).all()
    rng = np.random.default_rng(1000 * n_keys + S)
    stream, so, sl, sp = connections(c, S, rng)
    cap, env_cap = c.n + 10, 512
    exp_ix = oracle(stream, so, sl, sp, cap)
    n = exp_ix["total"]
    assert c.n // 3 < n < c.n and (exp_ix["heads"]["status"] == 1).sum() == 1
    bm, heads, idx, envs, n_env, sets, counts = gv.verify_frames_tally(
        stream, exp_ix["off"][:n], exp_ix["len"][:n], env_cap, peer=exp_ix["peer"][:n])
    st = heads["status"]
    # (with 256 replicas and a few connections nearly every vote names another replica than its connection's)
    many = n_keys == 4
    assert (st == 5).sum() > 5 and (st == 0).sum() > (n // 3 if many else 0)
    assert bitmap_to_bool(bm, n).sum() > (n // 4 if many else 0)
    for tile in (512, 0):
        gv.set_option(gv.OPT_INDEX_TILE, tile)
        try:
            r = gv.verify_streams_tally(stream, so, sl, cap, env_cap, seg_peer=sp, want_index=tile == 512)
        finally:
            gv.set_option(gv.OPT_INDEX_TILE, 0)
        assert r["n"] == n and r["n_frames"].tolist() == [n, 0]
        for k in ("status", "n_frames", "consumed", "first", "pad"):
            assert (r["seg_heads"][k] == exp_ix["heads"][k]).all(), k
        assert (r["bitmap"] == bm).all() and (r["heads"] == heads).all() and (r["env_idx"] == idx).all()
        assert (r["envelopes"] == envs).all() and (r["n_env"] == n_env).all()
        assert (r["signers"] == sets).all() and (r["counts"] == counts).all()
        if tile == 512:
            assert (r["off"] == exp_ix["off"][:n]).all() and (r["flen"] == exp_ix["len"][:n]).all()
    # frame_cap below the total: the first frame_cap frames, verified as those frames alone
    small = n - 50
    r = gv.verify_streams_tally(stream, so, sl, small, env_cap, seg_peer=sp)
    e = gv.verify_frames_tally(stream, exp_ix["off"][:small], exp_ix["len"][:small], env_cap,
                               peer=exp_ix["peer"][:small])
    assert r["n"] == small and r["n_frames"].tolist() == [n, 50]
    assert (r["bitmap"] == e[0]).all() and (r["heads"] == e[1]).all() and (r["env_idx"] == e[2]).all()
    assert (r["n_env"] == e[4]).all() and (r["signers"] == e[5]).all() and (r["counts"] == e[6]).all()
    # without peers nothing is bound to its connection
    r = gv.verify_streams_tally(stream, so, sl, cap, env_cap)
    e = gv.verify_frames_tally(stream, exp_ix["off"][:n], exp_ix["len"][:n], env_cap)
    assert (r["bitmap"] == e[0]).all() and (r["heads"] == e[1]).all() and (r["counts"] == e[6]).all()
    unbound, bound = (r["heads"]["status"] == 5).sum(), (st == 5).sum()
    assert unbound < bound if S < n_keys else unbound == bound  # (S >= n_keys: every signer has a connection)


class DevChain:
    """Device buffers of the whole chain: the index's, the frames' and the tally's, all poisoned and guarded."""

    def __init__(self, stream, so, sl, sp, cap, env_cap, n_keys):
        import torch
        from pbft_amd import FrameHead
        self.ix, self.out, self.cap, self.head = DevIndex(stream, so, sl, sp, cap), TallyOut(cap, env_cap, n_keys), cap, \
            FrameHead
        dev = torch.device("cuda", 0)
        self.rec = torch.full((cap * 160 + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.hd = torch.full((cap * 24 + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
        self.bm = torch.full(((cap + 63) // 64 * 8 + GUARD,), 0xC3, dtype=torch.uint8, device=dev)

    def frames_args(self):
        return dict(d_records=self.rec.data_ptr(), d_heads=self.hd.data_ptr(), d_bitmap=self.bm.data_ptr())

    def poison(self):
        self.ix.poison()
        self.rec.fill_(0xA5)
        self.hd.fill_(0x5A)
        self.bm.fill_(0xC3)
        for k, t in self.out.t.items():
            t.fill_(self.out.FILL[k])

    def read(self):
        n = self.cap
        rec, hd, bm = self.rec.cpu().numpy(), self.hd.cpu().numpy(), self.bm.cpu().numpy()
        assert (rec[n * 160:] == 0xA5).all() and (hd[n * 24:] == 0x5A).all(), "guard overwritten"
        assert (bm[(n + 63) // 64 * 8:] == 0xC3).all(), "guard overwritten"
        return dict(ix=self.ix.read(), rec=rec[:n * 160].copy(), hd=hd[:n * 24].copy(),
                    bm=bm[:(n + 63) // 64 * 8].copy(), tally=self.out.read())


def same_chain(a, b, where):
    for k in ("rec", "hd", "bm"):
        assert (a[k] == b[k]).all(), (where, k)
    for x, y, name in zip(a["tally"], b["tally"], ("env_idx", "envelopes", "n_env", "signers", "counts")):
        assert (x == y).all(), (where, name)


def run_chain(gv, d, n_keys, stream=0):
    a = d.ix.args()
    gv.verify_streams_tally_device(n_replicas=n_keys, stream=stream, **a, **d.frames_args(), **d.out.args())


@pytest.mark.parametrize("n_keys", [4, 256])
def test_device_chain(gv, cases, n_keys):
    """verify_streams_tally_device with frame_cap above the total, one enqueue without a host synchronisation inside:
    the index equals the oracle's, and records, heads, bitmap, env_idx, envelopes, n_env, signers and counts are byte
    for byte those of verify_frames_tally_device given the same padded index."""
    import torch
    c = cases[n_keys]
    assert gv.set_keys(c.pub).all()
    rng = np.random.default_rng(77 + n_keys)
    stream, so, sl, sp = connections(c, 5, rng)
    cap, env_cap = c.n + 33, 512
    exp_ix = oracle(stream, so, sl, sp, cap)
    assert exp_ix["total"] < c.n
    ts = torch.cuda.Stream()
    ref = DevChain(stream, so, sl, sp, cap, env_cap, n_keys)
    off, ln, pr = dev_bytes(exp_ix["off"]), dev_bytes(exp_ix["len"]), dev_bytes(exp_ix["peer"])
    gv.verify_frames_tally_device(d_stream=ref.ix.s.data_ptr(), stream_bytes=len(stream), d_off=off.data_ptr(),
                                  d_len=ln.data_ptr(), d_peer=pr.data_ptr(), n_replicas=n_keys, n=cap,
                                  stream=ts.cuda_stream, **ref.frames_args(), **ref.out.args())
    ts.synchronize()
    want = ref.read()
    hd = want["hd"].view(ref.head)
    assert (hd["status"][exp_ix["total"]:] == 6).all() and (hd["status"][:exp_ix["total"]] == 0).any()
    assert (want["tally"][0][exp_ix["total"]:] == 0xFFFFFFFF).all()  # padding frames are in no envelope
    d = DevChain(stream, so, sl, sp, cap, env_cap, n_keys)
    for tile in (512, 0):
        gv.set_option(gv.OPT_INDEX_TILE, tile)
        try:
            d.poison()
            torch.cuda.synchronize()
            run_chain(gv, d, n_keys, ts.cuda_stream)
            ts.synchronize()
        finally:
            gv.set_option(gv.OPT_INDEX_TILE, 0)
        got = d.read()
        check_index(got["ix"], exp_ix, ("chain", tile))
        same_chain(got, want, tile)


def test_chain_capture(gv, cases):
    """After reserve, group_reserve and index_reserve the device chain is captured into a graph on one stream and
    replayed three times with the stream's bytes and the segment table rewritten to other frame boundaries: each
    replay equals the eager result of the same input."""
    import torch
    c = cases[4]
    assert gv.set_keys(c.pub).all()
    S, cap, env_cap = 6, c.n + 20, 512
    inputs = [connections(c, S, np.random.default_rng(500 + i)) for i in range(3)]
    size = max(len(x[0]) for x in inputs) + 64
    inputs = [(np.concatenate([s, np.full(size - len(s), 0x7B, np.uint8)]), so, sl, sp) for s, so, sl, sp in inputs]
    assert len({tuple(x[1].tolist()) for x in inputs}) == 3  # three different segment tables
    gv.set_option(gv.OPT_INDEX_TILE, 512)
    try:
        gv.reserve(cap)
        gv.group_reserve(cap)
        gv.index_reserve(size, S)
        ts = torch.cuda.Stream()
        eager = []
        for x in inputs:
            d = DevChain(*x, cap, env_cap, 4)
            run_chain(gv, d, 4, ts.cuda_stream)
            ts.synchronize()
            eager.append(d.read())
            check_index(eager[-1]["ix"], oracle(*x, cap), "eager")
        assert any((eager[0]["ix"]["off"] != e["ix"]["off"]).any() for e in eager[1:])
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):  # d: the buffers of the last eager call
            run_chain(gv, d, 4, torch.cuda.current_stream().cuda_stream)
        for x, want in zip(inputs, eager):
            d.ix.s.copy_(dev_bytes(x[0], pad=(-len(x[0])) % 16))
            d.ix.so.copy_(dev_bytes(x[1]))
            d.ix.sl.copy_(dev_bytes(x[2]))
            d.poison()
            d.bm[:(cap + 63) // 64 * 8].fill_(0xFF)  # stale bits: a verify that ran ahead of the decode would keep some
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            got = d.read()
            check_index(got["ix"], want["ix"], "replay")
            same_chain(got, want, "replay")
    finally:
        gv.set_option(gv.OPT_INDEX_TILE, 0)


# ---- 8. argument errors ----
def test_argument_errors_write_nothing(gv, cases):
    import torch
    from pbft_amd import PbftError
    c = cases[4]
    assert gv.set_keys(c.pub).all()
    rng = np.random.default_rng(8)
    stream, so, sl, sp = connections(c, 3, rng)
    d = DevChain(stream, so, sl, sp, 64, 16, 4)
    good = d.ix.args()
    bads = (dict(d_stream=good["d_stream"] + 8), dict(d_stream=0), dict(d_seg_off=0), dict(d_seg_len=0),
            dict(d_seg_off=good["d_seg_off"] + 4), dict(d_seg_len=good["d_seg_len"] + 4), dict(d_off=0), dict(d_len=0),
            dict(d_off=good["d_off"] + 4), dict(d_len=good["d_len"] + 2), dict(d_peer=0), dict(d_seg_peer=0),
            dict(d_peer=good["d_peer"] + 1), dict(d_seg_heads=0), dict(d_seg_heads=good["d_seg_heads"] + 4),
            dict(d_n_frames=0), dict(d_n_frames=good["d_n_frames"] + 2), dict(n_segments=65537),
            dict(frame_cap=2**31 + 1), dict(stream_bytes=2**31 + 1))
    for bad in bads:
        with pytest.raises(PbftError) as e:
            gv.index_streams_device(**{**good, **bad})
        assert e.value.code == -1, bad
        with pytest.raises(PbftError) as e:
            gv.verify_streams_tally_device(n_replicas=4, **{**good, **bad}, **d.frames_args(), **d.out.args())
        assert e.value.code == -1, bad
    chain = {**good, **d.frames_args(), **d.out.args(), "n_replicas": 4}
    for bad in (dict(n_replicas=0), dict(env_cap=0), dict(d_records=0), dict(d_heads=chain["d_heads"] + 4),
                dict(d_bitmap=0), dict(d_env_idx=0), dict(d_n_env=0), dict(d_signers=0), dict(d_count=0)):
        with pytest.raises(PbftError) as e:
            gv.verify_streams_tally_device(**{**chain, **bad})
        assert e.value.code == -1, bad
    for bad in (dict(max_segments=65537), dict(max_stream_bytes=2**31 + 1)):
        with pytest.raises(PbftError) as e:
            gv.index_reserve(**{**dict(max_stream_bytes=1024, max_segments=4), **bad})
        assert e.value.code == -1, bad
    with pytest.raises(PbftError) as e:
        gv.verify_streams_tally(stream, so, sl, 64, 0, seg_peer=sp)  # env_cap = 0 with room for frames
    assert e.value.code == -1
    torch.cuda.synchronize()
    assert d.ix.untouched() and d.out.untouched()
    assert (d.rec.cpu().numpy() == 0xA5).all() and (d.hd.cpu().numpy() == 0x5A).all()
    assert (d.bm.cpu().numpy() == 0xC3).all()
    # legal: no segment, no room
    r = gv.verify_streams_tally(stream, so[:0], sl[:0], 0, 4)
    assert r["n"] == 0 and r["n_frames"].tolist() == [0, 0] and r["n_env"].tolist() == [0, 0]
