"""The replica's admission pass on the GPU (pbft_admit_device) against pbft_amd.admit_reference: exact equality of the
class per frame, the class counts, the clean bitmap, the residue list, its totals and the records' key indices, on
heads and records the frame decoder made from encoded streams, on the case list of tests/test_admit.py (synthetic
heads: every status value), and with the rows permuted inside every wave."""
import numpy as np
import pytest

import admit_cases
from test_gpu_frames import GUARD, dev_bytes
from test_gpu_verify import gv  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
FILL = dict(cls=0xA5, counts=0x5A, clean=0xC3, res=0x3C, n_res=0x96)


class AdmitOut:
    """The outputs of one call, poisoned, each followed by a poisoned guard."""

    def __init__(self, n, residue_cap):
        import torch
        self.n, self.cap = n, residue_cap
        self.size = dict(cls=n, counts=32, clean=(n + 63) // 64 * 8, res=16 * residue_cap, n_res=8)
        dev = torch.device("cuda", 0)
        self.t = {k: torch.full((self.size[k] + GUARD,), FILL[k], dtype=torch.uint8, device=dev) for k in self.size}

    def args(self):
        return dict(d_class=self.t["cls"].data_ptr(), d_counts=self.t["counts"].data_ptr(),
                    d_clean=self.t["clean"].data_ptr(), d_res=self.t["res"].data_ptr() if self.cap else 0,
                    d_n_res=self.t["n_res"].data_ptr())

    def read(self):
        from pbft_amd import AdmitResidue
        out = {}
        for k, t in self.t.items():
            a = t.cpu().numpy()
            assert (a[self.size[k]:] == FILL[k]).all(), ("guard overwritten", k)
            out[k] = a[:self.size[k]].copy()
        return dict(cls=out["cls"], counts=out["counts"].view(np.uint32), clean=out["clean"].view(np.uint64),
                    res=out["res"].view(AdmitResidue), n_res=out["n_res"].view(np.uint32))


def run_admit(gv, d_heads, rec, n, c, d_off=0, d_len=0, n_total=None):
    """One pbft_admit_device call on its own stream; returns the outputs and the records after it."""
    import torch
    out = AdmitOut(n, c["residue_cap"])
    d_nf = dev_bytes(np.array([n_total, 0], np.uint32)) if n_total is not None else None
    ts = torch.cuda.Stream()
    gv.admit_device(d_heads, rec.data_ptr(), n, c["view"], c["h"], c["log_window"], c["n_keys"], c["residue_cap"],
                    d_off=d_off, d_len=d_len, d_n_frames=d_nf.data_ptr() if d_nf is not None else 0,
                    stream=ts.cuda_stream, **out.args())
    ts.synchronize()
    r = rec.cpu().numpy()
    assert (r[n * 160:] == 0xA5).all(), "guard behind the records overwritten"
    return out.read(), r[:n * 160].reshape(n, 160).copy()


def same(got, want, where):
    for k in ("cls", "counts", "clean", "res", "n_res"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (where, k, got[k][:16], want[k][:16])


def check_records(before, after, keep, where):
    """Key index 0xFFFF at byte 150 of every row that is not clean; every other byte as it was."""
    exp = before.copy()
    exp[~keep, 150:152] = 0xFF
    assert np.array_equal(after, exp), (where, np.flatnonzero((after != exp).any(axis=1))[:8])


def synthetic(gv, c, rows):
    """The case's heads uploaded as they are, over records that hold each row's key index."""
    import pbft_amd
    n = len(rows)
    heads = admit_cases.to_heads(rows)
    off, flen = admit_cases.index_of(n)
    before = np.full((n, 160), 0x11, np.uint8)
    before[:, 150:152] = heads["key_idx"].astype("<u2").view(np.uint8).reshape(n, 2)
    rec = dev_bytes(before, pad=GUARD)
    rec[n * 160:] = 0xA5
    d_heads, d_off, d_len = dev_bytes(heads) if n else None, dev_bytes(off) if n else None, dev_bytes(flen) if n else None
    got, after = run_admit(gv, d_heads.data_ptr() if n else 0, rec, n, c, d_off.data_ptr() if n else 0,
                           d_len.data_ptr() if n else 0, n_total=c["n_total"])
    want = pbft_amd.admit_reference(heads, c["view"], c["h"], c["log_window"], c["n_keys"], c["residue_cap"],
                                    n_total=c["n_total"], off=off, flen=flen)
    same(got, want, c["name"])
    check_records(before, after, want["keep"], c["name"])
    return got


@pytest.mark.parametrize("c", admit_cases.cases(), ids=lambda c: c["name"])
def test_case_list(gv, c):
    """Every case of the CPU test (watermarks, a window past 2^64, view before window, every status value, both kinds,
    contested pairs and triples at rows 0/1, 63/64 and 255/256, padding, residue_cap below the residue, the largest
    key planes, random mixtures of 1, 63, 64, 65 and 4099 rows), and each again with its rows permuted inside every
    run of 64: the classes move with their rows."""
    got = synthetic(gv, c, c["rows"])
    rows, perm = admit_cases.permute_in_waves(c["rows"], seed=len(c["rows"]))
    moved = synthetic(gv, c, rows)
    if c["n_total"] is None:
        assert np.array_equal(moved["cls"], got["cls"][perm]) and np.array_equal(moved["counts"], got["counts"])


def test_no_rows(gv):
    """N = 0: zero counts, n_res = {0, 0}, the residue zeroed; nothing else is touched."""
    c = admit_cases.case("empty", [], residue_cap=5)
    got = synthetic(gv, c, [])
    assert not got["counts"].any() and not got["n_res"].any() and not got["res"]["frame"].any()


def frames_of(rows, n_keys, rng):
    """One encoded frame and one authenticated peer per row: an OK vote as the canonical signed vote of its signer on
    that signer's connection, status ESIGNER as a vote that names another replica than its connection's, kind 0 as a
    PrePrepare and every other status as a ClientRequest (the device decoder defers both)."""
    from pbft_amd import wire
    parts, peer = [], []
    for status, kind, view, seq, key in rows:
        dig, sig = rng.integers(0, 256, 64, dtype=np.uint8).tobytes(), rng.integers(0, 256, 64, dtype=np.uint8).tobytes()
        if status == admit_cases.OK and kind in (1, 2) and key < n_keys:
            m, p = wire.WireMsg(kind=kind, view=view, seq=seq, digest=dig, replica=key, sig=sig), key
        elif status == admit_cases.ESIGNER or (status == admit_cases.OK and kind in (1, 2)):
            m, p = wire.WireMsg(kind=1, view=view, seq=seq, digest=dig, replica=1, sig=sig), 0
        elif kind == 0 and status == admit_cases.OK:
            m, p = wire.WireMsg(kind=0, view=view, seq=seq, digest=dig, replica=key % n_keys, sig=sig,
                                operation=b"op", timestamp=7, client="127.0.0.1:8080"), key % n_keys
        else:
            m, p = wire.WireMsg(kind=3, operation=b"op", timestamp=7, client="127.0.0.1:8080"), 0
        body = wire.encode_json(m)
        parts.append(wire.uvi_encode(len(body)) + body)
        peer.append(p)
    return np.frombuffer(b"".join(parts), np.uint8), np.array(peer, np.uint16)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4099])
def test_decoded_streams(gv, n):
    """n frames encoded, indexed and decoded by the existing decoder, then admitted: equal to admit_reference over the
    decoded heads, the residue carrying the index's off / len, the non-clean records' key indices 0xFFFF and nothing
    else of the records changed.  The decoded heads are what the rows said: OK votes, ESIGNER, deferred frames."""
    import pbft_amd
    import torch
    from pbft_amd import wire
    from test_gpu_frames import DeviceFrames
    # (8,192 keys for ~60 % of the rows: at 4099 rows some votes are clean and some contested)
    c = admit_cases.case(f"decoded {n}", admit_cases.random_rows(n, 77 + n, h=7, log_window=256, n_keys=16), h=7,
                         log_window=256, n_keys=16, residue_cap=max(1, n // 3))
    stream, peer = frames_of(c["rows"], c["n_keys"], np.random.default_rng(n))
    off, flen, used = wire.frame_index(stream)
    assert len(off) == n and used == len(stream)
    d = DeviceFrames(stream, off, flen, peer=peer)
    ts = torch.cuda.Stream()
    gv.decode_frames_device(stream=ts.cuda_stream, **d.args(c["n_keys"]))
    ts.synchronize()
    before, heads, _ = d.read()
    want_status = [0 if (s == 0 and k in (1, 2)) else 5 if s == 5 else 6 for s, k, _, _, _ in c["rows"]]
    assert list(heads["status"]) == want_status
    got, after = run_admit(gv, d.hd.data_ptr(), d.rec, n, c, d.o.data_ptr(), d.l.data_ptr())
    want = pbft_amd.admit_reference(heads, c["view"], c["h"], c["log_window"], c["n_keys"], c["residue_cap"],
                                    off=off, flen=flen)
    same(got, want, n)
    check_records(before, after, want["keep"], n)
    if n == 4099:  # the mixture is one: every class but PAD, and the residue overflows its cap
        assert (want["counts"][:6] > 0).all() and want["n_res"][1] > 0
