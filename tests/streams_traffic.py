"""Traffic for the differential tests of pbft_replica_push_streams (tests/test_replica_streams.py without a GPU,
tests/test_gpu_replica_streams.py on one): what replica 0 of an n-replica network receives, as a list of calls, each a
list of segments (peer, frames, cut), each frame a spec that `materialize` signs and encodes.  View 1 (primary
1 % n), seqs 1..SEQS, log window WINDOW."""
import hashlib

import numpy as np

VIEW, WINDOW = 1, 8
PREPREPARE, PREPARE, COMMIT = 0, 1, 2


def op_of(seq, salt=b""):
    return b"op-%d" % seq + salt


def dig_of(seq, salt=b""):
    return hashlib.blake2b(op_of(seq, salt), digest_size=64).digest()


def vote(kind, seq, signer, view=VIEW, digest=None, replica=None, forged=False, sig_of=None, space=False):
    """A signed vote frame: `signer` signs, the frame names `replica` (default: the signer)."""
    return dict(kind=kind, view=view, seq=seq, digest=dig_of(seq) if digest is None else digest, signer=signer,
                replica=signer if replica is None else replica, forged=forged, sig_of=sig_of, space=space, raw=None)


def pre_prepare(seq, primary, view=VIEW, salt=b"", replica=None):
    f = vote(PREPREPARE, seq, primary, view=view, digest=dig_of(seq, salt), replica=replica)
    f["op"] = op_of(seq, salt)
    return f


def raw(body):
    return dict(raw=body)


def seg(peer, frames, cut=None, junk_at=None):
    """cut: None, 'varint' (the last frame loses everything behind its varint's first byte) or 'body' (its last 40
    bytes); junk_at: a framing error (an overlong varint) in front of frame junk_at."""
    return dict(peer=peer, frames=list(frames), cut=cut, junk_at=junk_at)


def silent_of(n):
    f = (n - 1) // 3
    return set(range(n - f, n))  # the last f replicas never send


def honest(n, seqs, forged=()):
    """Two phase-ordered calls with f silent replicas: the primary's PrePrepares and the backups' Prepares, then the
    Commits.  forged: (kind, seq, signer) whose signature is garbage."""
    p, quiet = VIEW % n, silent_of(n)
    live = [i for i in range(n) if i not in quiet]
    c1 = [seg(p, [pre_prepare(q, p) for q in seqs])]
    c1 += [seg(i, [vote(PREPARE, q, i, forged=(PREPARE, q, i) in forged) for q in seqs]) for i in live if i != p]
    c2 = [seg(i, [vote(COMMIT, q, i, forged=(COMMIT, q, i) in forged) for q in seqs]) for i in live]
    return [c1, c2]


def kinds(n, seqs):
    """name -> calls, each traffic kind of the issue on its own."""
    p = VIEW % n
    b = [i for i in range(n) if i != p]  # backups
    A, B = dig_of(1), dig_of(1, b"-other")
    s1 = seqs[0]
    late = honest(n, seqs[1:])  # (seqs[0] stays open, so the committed windows behind it are not collected)
    late.append([seg(i, [vote(k, q, i) for q in seqs[1:3] for k in (PREPARE, COMMIT)]) for i in (0, b[0])])
    edges = [vote(PREPARE, q, b[0]) for q in (0, 1, WINDOW, WINDOW + 1)] + \
            [vote(COMMIT, q, b[0]) for q in (0, WINDOW, WINDOW + 1, 2**64 - 1)]
    big = seg(b[0], [vote(PREPARE, q, b[0]) for q in seqs])
    return {
        "honest": honest(n, seqs),
        "forged": honest(n, seqs, forged={(PREPARE, seqs[0], b[0]), (COMMIT, seqs[1], p), (COMMIT, seqs[1], b[1])}),
        "equivocation": [[seg(p, [pre_prepare(1, p)]),
                          seg(b[0], [vote(PREPARE, 1, b[0], digest=d) for d in (A, B, A)]),
                          seg(b[1], [vote(PREPARE, 1, b[1])])]],
        "flood": [[seg(b[0], [vote(COMMIT, s1, b[0], digest=dig_of(s1, b"-%d" % j)) for j in range(6)])]],
        "repeat": [[seg(i, [vote(PREPARE, q, i) for q in seqs]) for i in b]] * 2,
        "pre-prepare with votes": [[seg(p, [pre_prepare(q, p) for q in seqs[:3]] +
                                        [vote(COMMIT, q, p) for q in seqs[:3]] + [pre_prepare(seqs[0], p, salt=b"-x")]),
                                    seg(b[0], [vote(PREPARE, q, b[0]) for q in seqs[:3]]),
                                    seg(b[1], [vote(PREPARE, q, b[1], digest=dig_of(q, b"-x")) for q in seqs[:3]])]],
        "relayed pre-prepare": [[seg(b[0], [pre_prepare(2, p), vote(PREPARE, 2, b[0])]),
                                 seg(b[1], [pre_prepare(2, b[1], replica=b[1])])]],
        "wrong replica": [[seg(b[0], [vote(PREPARE, 2, b[1]), vote(PREPARE, 2, b[0], replica=b[1]),
                                      vote(PREPARE, 2, b[0], replica=n + 3), vote(PREPARE, 3, b[0])])]],
        "stale view": [[seg(b[0], [vote(PREPARE, 2, b[0], view=0), vote(COMMIT, 2, b[0], view=VIEW + 1),
                                   vote(PREPARE, 99, b[0], view=7), vote(PREPARE, 2, b[0])])]],
        "watermarks": [[seg(b[0], edges)]],
        "committed round": late,
        "non-canonical": [[seg(b[0], [vote(PREPARE, 2, b[0], space=True), vote(COMMIT, 2, b[0])])]],
        "client request": [[seg(b[0], [raw(b'{"ClientRequest":{"operation":"x","timestamp":1,"client":"127.0.0.1:80"}}'),
                                       vote(PREPARE, 2, b[0]), raw(b"not json"), raw(b"")])]],
        "cut in varint": [[seg(big["peer"], big["frames"], cut="varint"), seg(b[1], [vote(PREPARE, 1, b[1])])]],
        "cut in body": [[seg(big["peer"], big["frames"], cut="body"), seg(b[1], [vote(PREPARE, 1, b[1])])]],
        "framing error": [[seg(big["peer"], big["frames"], junk_at=2), seg(b[1], [vote(PREPARE, 1, b[1])])]],
    }


def together(named):
    """Call k of every kind, merged into one call."""
    depth = max(len(c) for c in named.values())
    return [[s for c in named.values() if k < len(c) for s in c[k]] for k in range(depth)]


def envelope(kind, view, seq, digest):
    return b"PBFT" + bytes([kind]) + int(view).to_bytes(8, "little") + int(seq).to_bytes(8, "little") + digest


def materialize(calls, sign_batch):
    """calls -> list of (stream uint8 array, seg_off, seg_len, seg_peer); sign_batch(signers, envelopes (k, 85) uint8)
    -> (k, 64) uint8 signatures.  Segments lie in the stream with a few bytes of gap between them."""
    from pbft_amd import wire
    specs = [f for c in calls for s in c for f in s["frames"] if f["raw"] is None]
    uniq = {}
    for f in specs:
        uniq.setdefault((f["signer"], f["kind"], f["view"], f["seq"], f["digest"]), len(uniq))
    keys = list(uniq)
    env = np.frombuffer(b"".join(envelope(k, v, q, d) for _, k, v, q, d in keys), np.uint8).reshape(-1, 85)
    sigs = sign_batch(np.array([k[0] for k in keys], np.uint16), env) if keys else np.zeros((0, 64), np.uint8)
    out = []
    for c in calls:
        parts, off, length, peer, at = [], [], [], [], 0
        for s in c:
            bodies = []
            for f in s["frames"]:
                if f["raw"] is not None:
                    bodies.append(f["raw"])
                    continue
                sig = bytearray(sigs[uniq[(f["signer"], f["kind"], f["view"], f["seq"], f["digest"])]].tobytes())
                if f["forged"]:
                    sig[5] ^= 0x40
                extra = dict(operation=f["op"], timestamp=7, client="127.0.0.1:8080") if f["kind"] == PREPREPARE else {}
                body = wire.encode_json(wire.WireMsg(kind=f["kind"], view=f["view"], seq=f["seq"], digest=f["digest"],
                                                     replica=f["replica"], sig=bytes(sig), **extra))
                if f["space"]:
                    body = body.replace(b'"view":', b'"view": ', 1)
                bodies.append(body)
            frames = [wire.uvi_encode(len(x)) + x for x in bodies]
            if s["junk_at"] is not None:
                frames.insert(s["junk_at"], b"\xff" * 10 + b"\x01")
            data = b"".join(frames)
            if s["cut"] == "varint":
                data = data[:len(data) - len(frames[-1]) + 1]
            elif s["cut"] == "body":
                data = data[:-40]
            gap = b"\x7b" * (3 + len(parts) % 5)
            parts += [gap, data]
            off.append(at + len(gap))
            length.append(len(data))
            peer.append(s["peer"])
            at += len(gap) + len(data)
        out.append((np.frombuffer(b"".join(parts), np.uint8).copy(), np.array(off, np.uint64),
                    np.array(length, np.uint64), np.array(peer, np.uint16)))
    return out
