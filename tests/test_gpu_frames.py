"""GPU frame decoder (pbft_wire_decode_frames_device / pbft_verify_frames_device / pbft_verify_frames) against code
that is not under test: pbft_wire_decode_votes for statuses and rows, the C oracle for the bits.  GPU-signed votes of
n = 4 and n = 256 key sets whose decimal widths span 1..20 digits, so frame bodies start at every offset mod 16."""
import numpy as np
import pytest

from test_gpu_verify import coracle, gv, oracle_bits, seeds_for  # noqa: F401  (gv, coracle: fixtures)

pytestmark = pytest.mark.gpu
GUARD = 256  # poisoned bytes behind each device output
EDEFER, ESIGNER = 6, 5


def dev_bytes(a, pad=0):
    import torch
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    if pad:
        b = np.concatenate([b, np.full(pad, 0x7B, np.uint8)])  # ('{': bytes past the stream look like a frame start)
    return torch.from_numpy(b.copy()).to(torch.device("cuda", 0))


def wide(rng, n):
    """u64 values of every decimal width 1..20."""
    bits = rng.integers(0, 65, n)
    v = rng.integers(0, 2**64, n, dtype=np.uint64)
    return np.where(bits == 0, np.uint64(0), v >> (np.uint64(64) - np.maximum(bits, 1).astype(np.uint64)))


def signed_votes(gv, n_keys, n, seed, kinds=(1, 2)):
    """n valid signed messages of random replicas: dict of kind, view, seq, digest, replica, sig and the public keys."""
    rng = np.random.default_rng(seed)
    seeds = seeds_for(n_keys, tag=1000 + n_keys)
    kind = rng.choice(np.array(kinds, np.uint8), n)
    view, seq = wide(rng, n), wide(rng, n)
    dig = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    rep = rng.integers(0, n_keys, n).astype(np.uint16)
    env = np.zeros((n, 85), np.uint8)
    env[:, :4] = np.frombuffer(b"PBFT", np.uint8)
    env[:, 4] = kind
    env[:, 5:13] = view.astype("<u8").view(np.uint8).reshape(n, 8)
    env[:, 13:21] = seq.astype("<u8").view(np.uint8).reshape(n, 8)
    env[:, 21:] = dig
    R, S, pub = gv.sign(seeds, rep, env, 85)
    return dict(kind=kind, view=view, seq=seq, dig=dig, rep=rep, sig=np.concatenate([R, S], axis=1), pub=pub)


def body_of(v, i, **over):
    from pbft_amd import wire
    f = dict(kind=int(v["kind"][i]), view=int(v["view"][i]), seq=int(v["seq"][i]), digest=v["dig"][i].tobytes(),
             replica=int(v["rep"][i]), sig=v["sig"][i].tobytes())
    f.update(over)
    if f["kind"] in (0, 3):
        f.update(operation=b"op-%d" % i, timestamp=12345 + i, client="127.0.0.1:8080")
    return wire.encode_json(wire.WireMsg(**f))


N_CLASSES = 16


def mutate(v, i, cls, rng, n_replicas):
    """Frame i of the pool as mutation class cls: what a correct peer never sends and an adversary sends at will."""
    b = bytearray(body_of(v, i))
    at = int(rng.integers(len(b)))
    if cls == 0:
        b[at] ^= 1 << int(rng.integers(8))
    elif cls == 1:
        b.insert(at, int(rng.choice(np.frombuffer(b' 0a",}', np.uint8))))
    elif cls == 2:
        del b[at]
    elif cls == 3:
        del b[at:]
    elif cls == 4:  # uppercase hex
        j = next(j for j in range(60 + at % 200, len(b)) if chr(b[j]) in "abcdef")
        b[j] -= 32
    elif cls == 5:  # leading zero
        b = bytearray(bytes(b).replace(b'"view":', b'"view":0', 1))
    elif cls == 6:  # 2^64
        b = bytearray(body_of(v, i).replace(b'"view":%d,' % int(v["view"][i]), b'"view":18446744073709551616,', 1))
    elif cls == 7:  # whitespace: still this vote for serde
        j = [j for j in range(len(b)) if chr(b[j]) in ":,"][at % 9]
        b.insert(j + 1, 0x20)
    elif cls == 8:  # swapped fields: still this vote
        s = bytes(b)
        d0, r0, s0 = s.index(b',"digest"'), s.index(b',"replica"'), s.index(b',"signature"')
        b = bytearray(s[:d0] + s[r0:s0] + s[d0:r0] + s[s0:])
    elif cls == 9:  # an extra field: still this vote
        b = bytearray(bytes(b)[:-2] + b',"x":[1,{"y":null}]}}')
    elif cls == 10:  # a ClientRequest
        b = bytearray(body_of(v, i, kind=3, sig=None))
    elif cls == 11:  # an unsigned vote
        b = bytearray(body_of(v, i, sig=None))
    elif cls == 12:  # canonical, signed by nobody of this network
        b = bytearray(body_of(v, i, replica=n_replicas + int(rng.integers(3))))
    elif cls == 13:  # a digest that is not hex: serde reads the message, the vote decoder says EDIGEST
        s = bytes(b)
        d0 = s.index(b'"digest":"') + 10
        b = bytearray(s[:d0 + at % 128] + b"g" + s[d0 + at % 128 + 1:])
    elif cls == 14:  # a trailing newline
        b += b"\n"
    else:  # a signed PrePrepare whose signature (made for the vote) does not fit its kind-0 envelope
        b = bytearray(body_of(v, i, kind=0))
    return bytes(b)


def build_stream(v, n_replicas, seed, canonical_only=False):
    """One stream of len(v) frames: ~70 % canonical valid, ~10 % canonical with a corrupted signature or digest (still
    hex), ~20 % mutants of every class; signed PrePrepares (kind 0 in the pool) go through as they are.
    Returns (stream uint8, off, flen, canonical bool[n])."""
    from pbft_amd import wire
    rng = np.random.default_rng(seed)
    n = len(v["kind"])
    parts, canon = [], np.zeros(n, bool)
    for i in range(n):
        u = rng.random()
        if v["kind"][i] == 0:
            body = body_of(v, i)
        elif canonical_only or u < 0.7:
            body, canon[i] = body_of(v, i), True
        elif u < 0.8:
            sig, dig = v["sig"][i].copy(), v["dig"][i].copy()
            (sig if rng.random() < 0.5 else dig)[int(rng.integers(64))] ^= 1 << int(rng.integers(8))
            body, canon[i] = body_of(v, i, sig=sig.tobytes(), digest=dig.tobytes()), True
        else:
            body = mutate(v, i, (i + seed) % N_CLASSES, rng, n_replicas)
        parts.append(wire.uvi_encode(len(body)) + body)
    stream = np.frombuffer(b"".join(parts), np.uint8)
    off, flen, used = wire.frame_index(stream)
    assert len(off) == n and used == len(stream)
    return stream, off, flen, canon


class Expected:
    """What the host decoder and the oracle say about a stream of whole frames."""

    def __init__(self, coracle, pub, stream, n_replicas, peer=None):
        from pbft_amd import wire
        v = wire.decode_votes(stream.tobytes(), n_replicas)
        assert v.consumed == len(stream)
        n = len(v.status)
        self.status = v.status.copy()
        ok = np.nonzero(v.status == 0)[0]
        self.view, self.seq = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        self.kind, self.key = np.zeros(n, np.uint8), np.full(n, 0xFFFF, np.uint16)
        self.view[ok], self.seq[ok], self.kind[ok], self.key[ok] = v.view, v.seq, v.kind, v.key_idx
        self.records = np.zeros((n, 160), np.uint8)
        self.records[:, 150:152] = 0xFF
        if len(ok):
            self.records[ok] = wire.records_pack(v.R, v.S, v.key_idx, v.msg)
        self.bits = np.zeros(n, bool)
        if len(ok):
            self.bits[ok] = oracle_bits(coracle, pub, v.R, v.S, v.key_idx, v.msg, 85)
        if peer is not None:  # the peer rule: a vote (not a PrePrepare) naming another replica than its connection's
            bad = (self.status == 0) & (self.kind != 0) & (self.key != peer)
            self.status[bad] = ESIGNER
            self.view[bad] = self.seq[bad] = 0
            self.kind[bad], self.key[bad], self.bits[bad] = 0, 0xFFFF, False
            self.records[bad] = 0
            self.records[bad, 150:152] = 0xFF

    def check_heads(self, heads, flen, where, deferred_ok=False):
        st = heads["status"]
        if deferred_ok:  # the device form: every frame settled there agrees with the host; the rest is deferred
            assert ((st == self.status) | (st == EDEFER)).all(), where
        else:
            assert (st == self.status).all(), (where, np.nonzero(st != self.status)[0][:8])
        ok = st == 0
        for name, exp in (("view", self.view), ("seq", self.seq), ("kind", self.kind), ("key_idx", self.key)):
            assert (heads[name][ok] == exp[ok]).all(), (where, name)
        assert (heads["view"][~ok] == 0).all() and (heads["seq"][~ok] == 0).all() and (heads["kind"][~ok] == 0).all()
        assert (heads["key_idx"][~ok] == 0xFFFF).all(), where
        assert (heads["frame_len"] == flen).all(), where

    def check_records(self, records, heads, where):
        ok = heads["status"] == 0
        assert (records[ok] == self.records[ok]).all(), where
        assert (records[~ok][:, :150] == 0).all() and (records[~ok][:, 152:] == 0).all(), where
        assert (records[~ok][:, 150:152] == 0xFF).all(), where


class DeviceFrames:
    """A stream and its index on the device, poisoned outputs with guards behind them."""

    def __init__(self, stream, off, flen, peer=None):
        import torch
        from pbft_amd import FrameHead
        self.n, self.nbytes, self.head = len(off), len(stream), FrameHead
        dev = torch.device("cuda", 0)
        self.s = dev_bytes(stream, pad=(-len(stream)) % 16)  # readable up to the next multiple of 16, no further
        self.o, self.l = dev_bytes(off.astype(np.uint64)), dev_bytes(flen.astype(np.uint32))
        self.p = dev_bytes(peer.astype(np.uint16)) if peer is not None else None
        self.rec = torch.full((self.n * 160 + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.hd = torch.full((self.n * 24 + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
        self.bm = torch.full(((self.n + 63) // 64 * 8 + GUARD,), 0xC3, dtype=torch.uint8, device=dev)

    def args(self, n_replicas):
        return dict(d_stream=self.s.data_ptr(), stream_bytes=self.nbytes, d_off=self.o.data_ptr(),
                    d_len=self.l.data_ptr(), n_replicas=n_replicas, n=self.n, d_records=self.rec.data_ptr(),
                    d_heads=self.hd.data_ptr(), d_peer=self.p.data_ptr() if self.p is not None else 0)

    def read(self):
        from pbft_amd import bitmap_to_bool
        rec, hd, bm = self.rec.cpu().numpy(), self.hd.cpu().numpy(), self.bm.cpu().numpy()
        nr, nh, nb = self.n * 160, self.n * 24, (self.n + 63) // 64 * 8
        assert (rec[nr:] == 0xA5).all() and (hd[nh:] == 0x5A).all() and (bm[nb:] == 0xC3).all(), "guard overwritten"
        bits = bitmap_to_bool(bm[:nb].copy().view(np.uint64), self.n)
        return rec[:nr].reshape(self.n, 160).copy(), hd[:nh].copy().view(self.head), bits


@pytest.fixture(scope="module")
def pool4(gv):
    """344 signed messages of a 4-replica network; every 29th a signed PrePrepare."""
    v = signed_votes(gv, 4, 344, seed=4)
    w = signed_votes(gv, 4, 344, seed=5, kinds=(0,))
    pp = np.arange(344) % 29 == 7
    for k in ("kind", "view", "seq", "dig", "rep", "sig"):
        v[k][pp] = w[k][pp]
    return v


def test_frames_match_host_decode(gv, coracle, pool4):
    """verify_frames on 1, 63, 64 and 200 frames (one lane, a partial wave, a full wave, several waves and a tail):
    statuses equal pbft_wire_decode_votes', records of OK frames equal records_pack of the host rows, bit f = (OK and
    the oracle accepts)."""
    from pbft_amd import bitmap_to_bool
    assert gv.set_keys(pool4["pub"]).all()
    lo, seen, start16 = 0, set(), set()
    for n in (1, 63, 64, 200):
        v = {k: a[lo:lo + n] for k, a in pool4.items() if k != "pub"}
        lo += n
        stream, off, flen, canon = build_stream(v, 4, seed=n)
        exp = Expected(coracle, pool4["pub"], stream, 4)
        bm, heads, records = gv.verify_frames(stream, off, flen)
        exp.check_heads(heads, flen, n)
        exp.check_records(records, heads, n)
        got = bitmap_to_bool(bm, n)
        assert (got == exp.bits).all(), (n, np.nonzero(got != exp.bits)[0][:8])
        assert (exp.status[canon] == 0).all()
        seen |= set(exp.status.tolist())
        start16 |= set((off % 16).tolist())
        if n == 200:  # the mix is what it claims: valid votes, forged ones, settled mutants of either outcome
            assert exp.bits[canon].sum() > 100 and (~exp.bits[canon]).sum() > 5
            assert (exp.bits & ~canon).sum() > 5 and ((exp.status == 0) & (exp.kind == 0)).any()
    assert seen == {0, 1, 2, 3, 4, 5} and start16 == set(range(16))


def test_decode_device_only(gv, coracle, pool4):
    """decode_frames_device alone: canonical frames are never deferred (0 of a canonical-only input), every other frame
    is deferred or has the host's status, non-OK records are zero with key index 0xFFFF."""
    import torch
    v = {k: a[:200] for k, a in pool4.items() if k != "pub"}
    v["kind"] = np.where(v["kind"] == 0, 1, v["kind"]).astype(np.uint8)  # (the signatures do not matter here)
    for canonical_only in (True, False):
        stream, off, flen, canon = build_stream(v, 4, seed=11, canonical_only=canonical_only)
        exp = Expected(coracle, pool4["pub"], stream, 4)
        d = DeviceFrames(stream, off, flen)
        ts = torch.cuda.Stream()
        gv.decode_frames_device(stream=ts.cuda_stream, **d.args(4))
        ts.synchronize()
        records, heads, _ = d.read()
        exp.check_heads(heads, flen, canonical_only, deferred_ok=True)
        exp.check_records(records, heads, canonical_only)
        deferred = heads["status"] == EDEFER
        assert not deferred[canon].any()
        if canonical_only:
            assert canon.all() and deferred.sum() == 0 and (heads["status"] == 0).all()
        else:
            assert deferred.sum() > 20 and (exp.status[deferred] == 0).any() and (exp.status[deferred] != 0).any()
            assert (heads["status"] == ESIGNER).any()  # canonical votes of replica >= n_replicas: settled on the device


def test_frames_gapped_and_bounds(gv, coracle, pool4):
    """Frames with gaps between them and in reverse order; one frame ending one byte past the stream; the last frame
    ending exactly at a stream_bytes that is no multiple of 16; lengths 335, 336, 379 and 380."""
    import torch
    from pbft_amd import PbftError, bitmap_to_bool, wire
    assert gv.set_keys(pool4["pub"]).all()
    rng = np.random.default_rng(33)
    votes = [i for i in range(150) if pool4["kind"][i] != 0]
    bodies = [body_of(pool4, i) for i in votes[:130]]
    small = body_of(pool4, votes[130], kind=2, view=1, seq=2)          # 336: the signature no longer fits, still OK
    large = body_of(pool4, votes[131], kind=1, view=2**64 - 1, seq=10**19, replica=65535)  # 379: ESIGNER (n = 4)
    assert len(small) == 336 and len(large) == 379
    bodies += [small, small[:5] + small[6:], large, large + b" "]  # 336, 335 ("Comit"), 379, 380
    order = rng.permutation(len(bodies))
    chunks, off, flen, at = [], np.zeros(len(bodies), np.uint64), np.zeros(len(bodies), np.uint32), 0
    for j in order[::-1]:  # laid out in reverse of their frame numbers' shuffle, random gaps (0..40 bytes) between
        gap = bytes(rng.integers(0, 256, int(rng.integers(0, 41)), dtype=np.uint8))
        chunks += [gap, bodies[j]]
        off[j], flen[j], at = at + len(gap), len(bodies[j]), at + len(gap) + len(bodies[j])
    stream = np.frombuffer(b"".join(chunks), np.uint8)
    if len(stream) % 16 == 0:
        stream, off = np.concatenate([np.zeros(3, np.uint8), stream]), off + np.uint64(3)
    assert len(stream) % 16 != 0 and (off + flen).max() == len(stream)  # the last frame ends the stream
    n = len(bodies)
    # the host's word on each body, as one packed stream of the same frames
    packed = np.frombuffer(b"".join(wire.uvi_encode(len(b)) + b for b in bodies), np.uint8)
    exp = Expected(coracle, pool4["pub"], packed, 4)
    assert exp.status[n - 4:].tolist() == [0, 1, ESIGNER, ESIGNER]
    dev_status = exp.status.copy()  # what the device settles: the lengths outside 336..379 are deferred unread
    dev_status[[n - 3, n - 1]] = EDEFER
    bm, heads, records = gv.verify_frames(stream, off, flen)
    exp.check_heads(heads, flen, "host form")
    exp.check_records(records, heads, "host form")
    assert (bitmap_to_bool(bm, n) == exp.bits).all() and exp.bits.sum() >= 125
    # device form: the same, the non-canonical ones (335, 380) deferred without being read
    d = DeviceFrames(stream, off, flen)
    ts = torch.cuda.Stream()
    gv.verify_frames_device(d_bitmap=d.bm.data_ptr(), stream=ts.cuda_stream, **d.args(4))
    ts.synchronize()
    records, heads, bits = d.read()
    exp.check_heads(heads, flen, "device form", deferred_ok=True)
    exp.check_records(records, heads, "device form")
    assert (heads["status"] == dev_status).all() and dev_status[n - 4:].tolist() == [0, EDEFER, ESIGNER, EDEFER]
    assert (heads["status"][:n - 4] == 0).all() and (bits == exp.bits).all()
    # one byte past the end: marked on the device (and not read), refused by the host form
    last = int(np.argmax(off + flen))
    off2 = off.copy()
    off2[last] += 1
    d = DeviceFrames(stream, off2, flen)
    gv.verify_frames_device(d_bitmap=d.bm.data_ptr(), stream=ts.cuda_stream, **d.args(4))
    ts.synchronize()
    records, heads, bits = d.read()
    assert heads["status"][last] == EDEFER and not bits[last] and (records[last, :150] == 0).all()
    keep = np.arange(n) != last
    assert (heads["status"][keep] == dev_status[keep]).all()
    assert (bits[keep] == exp.bits[keep]).all()
    with pytest.raises(PbftError) as e:
        gv.verify_frames(stream, off2, flen)
    assert e.value.code == -1
    for bad in (dict(n_replicas=0), dict(n_replicas=65536), dict(d_stream=d.s.data_ptr() + 8),
                dict(d_records=d.rec.data_ptr() + 8), dict(d_heads=d.hd.data_ptr() + 4), dict(d_off=0)):
        with pytest.raises(PbftError) as e:
            gv.decode_frames_device(**{**d.args(4), **bad})
        assert e.value.code == -1, bad
    bm, heads, records = gv.verify_frames(b"", np.zeros(0, np.uint64), np.zeros(0, np.uint32))  # N = 0: nothing
    assert len(bm) == 0 and len(heads) == 0


def test_peer_rule(gv, coracle, pool4):
    """With a peer per frame, a valid vote naming another replica is ESIGNER and bit 0; without, it is OK."""
    import torch
    from pbft_amd import bitmap_to_bool
    assert gv.set_keys(pool4["pub"]).all()
    v = {k: a[100:230] for k, a in pool4.items() if k != "pub"}
    n = 130
    stream, off, flen, canon = build_stream(v, 4, seed=2)
    rng = np.random.default_rng(9)
    peer = np.where(rng.random(n) < 0.7, v["rep"], (v["rep"] + 1) % 4).astype(np.uint16)
    free, bound = Expected(coracle, pool4["pub"], stream, 4), Expected(coracle, pool4["pub"], stream, 4, peer)
    moved = (free.status == 0) & (bound.status == ESIGNER)
    assert moved.sum() > 15 and free.bits[moved].sum() > 10 and (moved & ~canon).any()
    assert ((free.status == 0) & (free.kind == 0) & (free.key != peer)).any()  # a PrePrepare is not bound to the peer
    for exp, p in ((free, None), (bound, peer)):
        bm, heads, records = gv.verify_frames(stream, off, flen, peer=p)
        exp.check_heads(heads, flen, p is None)
        exp.check_records(records, heads, p is None)
        assert (bitmap_to_bool(bm, n) == exp.bits).all()
        d = DeviceFrames(stream, off, flen, p)
        ts = torch.cuda.Stream()
        gv.verify_frames_device(d_bitmap=d.bm.data_ptr(), stream=ts.cuda_stream, **d.args(4))
        ts.synchronize()
        records, heads, bits = d.read()
        exp.check_heads(heads, flen, p is None, deferred_ok=True)
        settled = heads["status"] != EDEFER
        assert settled[canon].all() and (bits[settled] == exp.bits[settled]).all() and not bits[~settled].any()


def test_frames_capture(gv, pool4):
    """reserve, one eager verify_frames_device, then decode + verify captured as one chain into a graph and replayed
    on changed input in the same buffers: bitmap and heads equal the eager results."""
    import torch
    assert gv.set_keys(pool4["pub"]).all()
    v = {k: a[:150] for k, a in pool4.items() if k != "pub"}
    stream_a, off, flen, canon = build_stream(v, 4, seed=3, canonical_only=True)
    n = len(off)
    stream_b = stream_a.copy()  # the same index: some signatures forged (still hex), some frames broken
    for f in range(0, n, 3):
        at = int(off[f]) + int(flen[f]) - 10
        stream_b[at] = ord("0") if stream_b[at] != ord("0") else ord("1")
    for f in range(1, n, 7):
        stream_b[int(off[f]) + 3] = ord("X")
    gv.reserve(n)
    eager = {}
    ts = torch.cuda.Stream()
    for name, s in (("b", stream_b), ("a", stream_a)):
        d = DeviceFrames(s, off, flen)
        gv.verify_frames_device(d_bitmap=d.bm.data_ptr(), stream=ts.cuda_stream, **d.args(4))
        ts.synchronize()
        eager[name] = d.read()
    assert (eager["a"][1]["status"][canon] == 0).all() and eager["a"][2].sum() > 100
    assert (eager["b"][1]["status"][1::7] == EDEFER).all() and not eager["b"][2][0::3].any()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # d: the buffers of the last eager call (input a)
        gv.verify_frames_device(d_bitmap=d.bm.data_ptr(), stream=torch.cuda.current_stream().cuda_stream, **d.args(4))
    for name, s in (("a", stream_a), ("b", stream_b)):
        d.s.copy_(dev_bytes(s, pad=(-len(s)) % 16))
        d.rec[:n * 160].fill_(0xA5)
        d.hd[:n * 24].fill_(0x5A)
        d.bm[:(n + 63) // 64 * 8].fill_(0xFF)  # stale bits: a verify that ran ahead of the decode would keep some
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        records, heads, bits = d.read()
        assert (heads == eager[name][1]).all() and (bits == eager[name][2]).all(), name
        assert (records == eager[name][0]).all(), name


def test_frames_one_round(gv):
    """2^14 canonical votes (n = 256, 64 sequence numbers, ~1 % forged): the bitmap of verify_frames equals
    verify_records of the host-decoded records.  The one test at a size where the comb runs its one-lane path."""
    from pbft_amd import bitmap_to_bool, wire
    n_keys, n_seq = 256, 64
    n = n_keys * n_seq
    rng = np.random.default_rng(14)
    seeds = seeds_for(n_keys, tag=1256)
    seq = np.repeat(np.arange(1000, 1000 + n_seq, dtype=np.uint64), n_keys)
    rep = np.tile(np.arange(n_keys, dtype=np.uint16), n_seq)
    kind = np.where(seq % 2 == 0, 1, 2).astype(np.uint8)
    view = np.full(n, 7, np.uint64)
    dseq = rng.integers(0, 256, (n_seq, 64), dtype=np.uint8)
    dig = np.repeat(dseq, n_keys, axis=0)
    env = np.zeros((n, 85), np.uint8)
    env[:, :4] = np.frombuffer(b"PBFT", np.uint8)
    env[:, 4] = kind
    env[:, 5:13] = view.view(np.uint8).reshape(n, 8)
    env[:, 13:21] = seq.view(np.uint8).reshape(n, 8)
    env[:, 21:] = dig
    R, S, pub = gv.sign(seeds, rep, env, 85)
    assert gv.set_keys(pub).all()
    sig = np.concatenate([R, S], axis=1)
    forged = rng.choice(n, n // 100, replace=False)
    sig[forged, rng.integers(0, 64, len(forged))] ^= 0x10
    stream = wire.encode_votes(kind, view, seq, dig, rep.astype(np.uint32), sig)
    off, flen, used = wire.frame_index(stream)
    assert len(off) == n and used == len(stream)
    hv = wire.decode_votes(stream.tobytes(), n_keys, max_frames=n)
    assert (hv.status == 0).all() and (hv.msg == env).all()
    host_records = wire.records_pack(hv.R, hv.S, hv.key_idx, hv.msg)
    exp = bitmap_to_bool(gv.verify_records(host_records), n)
    assert exp.sum() == n - len(forged) and not exp[forged].any()
    bm, heads, records = gv.verify_frames(stream, off, flen, peer=rep)
    assert (heads["status"] == 0).all() and (records == host_records).all()
    assert (heads["seq"] == seq).all() and (heads["key_idx"] == rep).all() and (heads["kind"] == kind).all()
    assert (bitmap_to_bool(bm, n) == exp).all()
