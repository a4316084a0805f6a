"""The replica's egress without a GPU: the outbox that pbft_replica's decided events fill, and
pbft_replica_emit_frames under a signer override (the C oracle's RFC 8032 signatures encoded by
pbft_wire_encode_votes; tests/egress_sim.py).  The verifier and the digest are the overrides of tests/replica_sim.py."""
import ctypes
import hashlib

import numpy as np

import egress_sim as E
from pbft_amd import wire
from replica_sim import (EV_COMMITTED, EV_PRE_PREPARED, EV_PREPARED, KIND_COMMIT, KIND_PREPARE, KIND_PREPREPARE, Cluster,
                         Event)
from test_replica_streams import SegHead, bind as bind_streams

VIEW = 1
OP = b"testOperation"
D = hashlib.blake2b(OP, digest_size=64).digest()


class Net(Cluster):
    """A 4-replica cluster whose replicas may sign through the oracle override."""

    def __init__(self, signers=()):
        super().__init__(4)
        E.bind(self.L)
        bind_streams(self.L)
        self.signers = {}
        for i in signers:
            self.signers[i] = E.OracleSigner(self.o, self.seeds[i])
            self.signers[i].install(self.L, self.reps[i])

    def votes(self, i, kind, seqs, senders):
        for q in seqs:
            for s in senders:
                assert self.L.pbft_replica_push(self.reps[i], kind, VIEW, q, D, s, self.sign(s, kind, VIEW, q, D)) == 1

    def decoded(self, stream):
        v = wire.decode_votes(stream.tobytes(), self.n)
        assert v.consumed == len(stream) and (v.status == 0).all()
        return v

    def verifies(self, i, v):
        n = len(v.R)
        acc = np.zeros(n, np.uint8)
        K = np.full(n, i, np.uint16)
        self.o.oracle_verify_batch(self.keys_np.ctypes.data, self.n, v.R.ctypes.data, v.S.ctypes.data, K.ctypes.data,
                                   v.msg.ctypes.data, 85, 85, n, acc.ctypes.data, 1)
        return acc.astype(bool)


def expected_votes(events):
    """One Prepare per PRE_PREPARED and one Commit per PREPARED, in event order: (kind, view, seq)."""
    return [(KIND_PREPARE if k == EV_PRE_PREPARED else KIND_COMMIT, v, q) for v, q, k in events
            if k in (EV_PRE_PREPARED, EV_PREPARED)]


def test_outbox_off_by_default():
    a, b = Net(), Net(signers=[2])
    try:
        ev = []
        for c in (a, b):
            for q in (1, 2):
                assert c.pre_prepare(2, VIEW, q, OP) == 1
            c.votes(2, KIND_PREPARE, (1, 2), (0, 1, 3))
            c.votes(2, KIND_COMMIT, (1,), (0, 1, 3))
            ev.append(c.flush(2, force=1))
        assert ev[0] == ev[1] and len(ev[0]) == 5  # the same events with and without a signer
        rc, stream, n, votes = E.emit(a.L, a.reps[2])
        assert (rc, n, votes) == (0, 0, 0)
        assert E.egress_stats(a.L, a.reps[2]) == dict(queued=0, emitted=0, calls=0, loopback_pushed=0, emit_ns=0)
        assert E.egress_stats(b.L, b.reps[2])["queued"] == 4
        sa, sb = a.stats(2), b.stats(2)
        assert all(sa[k] == sb[k] for k in sa if not k.endswith("_ns")), (sa, sb)
    finally:
        a.close()
        b.close()


def test_events_to_frames():
    c = Net(signers=[2])
    try:
        seqs = (1, 2, 3, 5)
        events = []
        for q in seqs:
            assert c.pre_prepare(2, VIEW, q, OP) == 1
        events += c.flush(2, force=1)
        c.votes(2, KIND_PREPARE, seqs[1:], (0, 3))
        events += c.flush(2, force=1)
        c.votes(2, KIND_PREPARE, seqs[:1], (0, 1, 3))
        events += c.flush(2, force=1)
        want = expected_votes(events)
        assert len(want) == 8 and E.egress_stats(c.L, c.reps[2])["queued"] == 8
        rc, stream, n, votes = E.emit(c.L, c.reps[2])
        assert rc == 0 and votes == 8 and n == len(stream)
        v = c.decoded(stream)
        assert list(zip(v.kind.tolist(), v.view.tolist(), v.seq.tolist())) == want
        assert (v.key_idx == 2).all() and (v.msg[:, 21:] == np.frombuffer(D, np.uint8)).all()
        assert c.verifies(2, v).all()
        st = E.egress_stats(c.L, c.reps[2])
        assert (st["queued"], st["emitted"], st["calls"], st["loopback_pushed"]) == (0, 8, 1, 0)
        assert c.signers[2].calls == 1
    finally:
        c.close()


def test_cap_too_small_leaves_the_outbox():
    c = Net(signers=[2])
    try:
        assert c.pre_prepare(2, VIEW, 1, OP) == 1
        c.votes(2, KIND_PREPARE, (1,), (0, 3))
        c.flush(2, force=1)
        need, nv = ctypes.c_size_t(), ctypes.c_uint64(7)
        assert c.L.pbft_replica_emit_frames(c.reps[2], 0, None, 0, ctypes.byref(need), ctypes.byref(nv)) == 0
        query = need.value
        assert query > 2 * 338 - 1 and nv.value == 0
        rc, stream, n, votes = E.emit(c.L, c.reps[2], cap=query - 1)
        assert (rc, n, votes) == (E.EINVAL, query, 0)
        assert E.egress_stats(c.L, c.reps[2])["queued"] == 2 and c.signers[2].calls == 0
        rc, stream, n, votes = E.emit(c.L, c.reps[2], cap=query)
        assert (rc, n, votes) == (0, query, 2) and len(stream) == query
        assert len(c.decoded(stream).R) == 2
        rc, stream, n, votes = E.emit(c.L, c.reps[2], cap=query)
        assert (rc, n, votes) == (0, 0, 0)
    finally:
        c.close()


def test_wrong_seed_leaves_the_outbox_off():
    c = Net()
    try:
        # no GPU context here: no seed can be installed; on the GPU the same call refuses a seed of another key
        assert c.L.pbft_replica_set_signing_seed(c.reps[2], c.seeds[3]) == E.EINVAL
        assert c.pre_prepare(2, VIEW, 1, OP) == 1
        assert c.flush(2, force=1) == [(VIEW, 1, EV_PRE_PREPARED)]
        assert E.egress_stats(c.L, c.reps[2])["queued"] == 0
        assert E.emit(c.L, c.reps[2])[3] == 0
        assert c.L.pbft_replica_set_signing_seed(c.reps[2], None) == 0
    finally:
        c.close()


def test_commit_of_a_window_collected_in_the_same_flush():
    c = Net(signers=[2])
    try:
        assert c.pre_prepare(2, VIEW, 1, OP) == 1
        c.votes(2, KIND_PREPARE, (1,), (0, 3))
        c.votes(2, KIND_COMMIT, (1,), (0, 1, 3))
        ev = c.flush(2, force=1)
        assert [k for _, _, k in ev] == [EV_PRE_PREPARED, EV_PREPARED, EV_COMMITTED]
        st = c.stats(2)
        assert st["windows_gc"] == 1 and st["live_windows"] == 0 and st["low_watermark"] == 1  # the window is gone
        rc, stream, n, votes = E.emit(c.L, c.reps[2])
        v = c.decoded(stream)
        assert list(zip(v.kind.tolist(), v.seq.tolist())) == [(KIND_PREPARE, 1), (KIND_COMMIT, 1)]
        assert (v.msg[:, 21:] == np.frombuffer(D, np.uint8)).all() and c.verifies(2, v).all()
    finally:
        c.close()


def test_loopback_counts_the_replicas_own_vote():
    c = Net(signers=[2])
    try:
        assert c.pre_prepare(2, VIEW, 1, OP) == 1
        c.votes(2, KIND_PREPARE, (1,), (0,))  # 2f - 1 other replicas
        assert c.flush(2, force=1) == [(VIEW, 1, EV_PRE_PREPARED)]
        assert c.flush(2, force=1) == [] and c.L.pbft_replica_prepared(c.reps[2], VIEW, 1) == 0
        rc, stream, n, votes = E.emit(c.L, c.reps[2], flags=E.EMIT_LOOPBACK)
        assert rc == 0 and votes == 1
        assert E.egress_stats(c.L, c.reps[2])["loopback_pushed"] == 1
        before = c.stats(2)["accepted"]
        assert c.flush(2, force=1) == [(VIEW, 1, EV_PREPARED)]  # its own Prepare, verified like anyone's
        assert c.stats(2)["accepted"] == before + 1 and c.L.pbft_replica_prepared(c.reps[2], VIEW, 1) == 1
    finally:
        c.close()


def test_closed_loop_of_four_replicas():
    """Only the primary's PrePrepares are signed by the test; every vote any replica receives is what another
    replica's emit_frames produced, delivered through pbft_replica_push_streams."""
    c = Net(signers=[0, 1, 2, 3])
    try:
        seqs = (1, 2, 3)
        p = c.primary(VIEW)
        pp = b"".join(wire.encode_frame(wire.WireMsg(kind=wire.PREPREPARE, view=VIEW, seq=q, digest=D, replica=p,
                                                     sig=c.sign(p, KIND_PREPREPARE, VIEW, q, D), operation=OP,
                                                     timestamp=q, client="127.0.0.1:8080")) for q in seqs)
        wires = {i: {p: pp} for i in range(c.n)}  # wires[dst][src]: bytes on the connection src -> dst
        events = {i: [] for i in range(c.n)}
        for _ in range(8):
            if not any(wires[i] for i in wires):
                break
            sent = {}
            for i in range(c.n):
                segs, wires[i] = sorted(wires[i].items()), {}
                stream = np.frombuffer(b"".join(b for _, b in segs) + bytes(16), np.uint8).copy()
                length = np.array([len(b) for _, b in segs], np.uint64)
                off = (np.cumsum(length) - length).astype(np.uint64)
                peer = np.array([s for s, _ in segs], np.uint16)
                heads = (SegHead * max(1, len(segs)))()
                a, b, ne, ev = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32(), (Event * 64)()
                assert c.L.pbft_replica_push_streams(c.reps[i], stream.ctypes.data, int(length.sum()), off.ctypes.data,
                                                     length.ctypes.data, peer.ctypes.data, len(segs), heads,
                                                     ctypes.byref(a), ctypes.byref(b), ev, 64, ctypes.byref(ne)) == 0
                assert all(h.consumed == n for h, n in zip(heads, length)) and b.value == 0
                events[i] += [(e.view, e.seq, e.kind) for e in ev[:ne.value]]
                rc, out, n, votes = E.emit(c.L, c.reps[i], flags=E.EMIT_LOOPBACK)
                assert rc == 0
                if votes:
                    sent[i] = out.tobytes()
            for src, data in sent.items():
                for dst in range(c.n):
                    if dst != src:
                        wires[dst][src] = data
        for i in range(c.n):
            for q in seqs:
                assert (VIEW, q, EV_COMMITTED) in events[i], (i, q, events[i])
                assert c.L.pbft_replica_committed_local(c.reps[i], VIEW, q) == 1
            st = E.egress_stats(c.L, c.reps[i])
            assert st["emitted"] == 2 * len(seqs) == st["loopback_pushed"] and st["queued"] == 0
    finally:
        c.close()
