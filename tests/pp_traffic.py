"""PrePrepare traffic and frames for tests/test_pp.py (without a GPU) and tests/test_gpu_pp.py (on one).

`kinds` is replica traffic in the shape of tests/streams_traffic.py (whose `materialize` signs and encodes it): what
replica 0 receives when the primary's PrePrepares are honest, relayed, misattributed, inconsistent, repeated, stale,
outside the window, escaped, or interleaved with its votes.  `corpus` is the decoder's differential corpus: frames from
the encoder at the edges of the canonical form, and mutations of three of them."""
import hashlib

import numpy as np

import streams_traffic as T

OP_MAX = 3072
ALPHABET = bytes(c for c in range(0x20, 0x7F) if c not in b'"\\')


def in_alphabet(s):
    return all(c in ALPHABET for c in bytes(s))


def pp(seq, primary, op=None, view=T.VIEW, replica=None, digest=None):
    """A signed PrePrepare: `primary` signs the claimed digest (default: that of the operation)."""
    f = T.pre_prepare(seq, primary, view=view, replica=replica)
    if op is not None:
        f["op"] = op
        f["digest"] = hashlib.blake2b(op, digest_size=64).digest()
    if digest is not None:
        f["digest"] = digest
    return f


def canonical(f):
    """What the spec says about a frame spec: the encoder's form of it is the canonical PrePrepare."""
    return f.get("raw") is None and f["kind"] == T.PREPREPARE and in_alphabet(f["op"]) and len(f["op"]) <= OP_MAX \
        and not f["space"]


ESCAPED = b'say "hi"\\ to\tall'  # a quote, a backslash and a control byte: the encoder escapes all three


def kinds(n, seqs):
    p = T.VIEW % n
    b = [i for i in range(n) if i != p]
    s1, s2 = seqs[0], seqs[1]
    long_op = bytes(ALPHABET[i % len(ALPHABET)] for i in range(300))
    rounds = T.honest(n, seqs)
    escaped = T.honest(n, seqs)
    escaped[0][0] = T.seg(p, [pp(q, p, op=ESCAPED + b"%d" % q) if q % 2 else pp(q, p) for q in seqs])
    escaped[0][1:] = [T.seg(s["peer"], [T.vote(T.PREPARE, f["seq"], f["signer"],
                                               digest=hashlib.blake2b(ESCAPED + b"%d" % f["seq"], digest_size=64).digest()
                                               if f["seq"] % 2 else None) for f in s["frames"]])
                      for s in escaped[0][1:]]
    escaped[1] = [T.seg(s["peer"], [T.vote(T.COMMIT, f["seq"], f["signer"],
                                           digest=hashlib.blake2b(ESCAPED + b"%d" % f["seq"], digest_size=64).digest()
                                           if f["seq"] % 2 else None) for f in s["frames"]]) for s in escaped[1]]
    between = T.honest(n, seqs)
    between[0][0] = T.seg(p, [x for q in seqs for x in (T.vote(T.COMMIT, q, p), pp(q, p), T.vote(T.PREPARE, q, p))])
    return {
        "honest": rounds,
        "long operation": [[T.seg(p, [pp(s1, p, op=long_op), pp(s2, p, op=b"")])]],
        "relayed": [[T.seg(b[0], [pp(s1, p), T.vote(T.PREPARE, s1, b[0])]), T.seg(p, [pp(s2, p)])]],
        "non-primary replica": [[T.seg(b[1], [pp(s1, b[1], replica=b[1])]), T.seg(p, [pp(s1, p, replica=b[0]), pp(s2, p)])]],
        "digest mismatch": [[T.seg(p, [pp(s1, p, digest=T.dig_of(s1, b"-other")), pp(s2, p)])]],
        "two for one seq": [[T.seg(p, [pp(s1, p), pp(s1, p, op=T.op_of(s1, b"-x")), pp(s2, p)])]],
        "same twice": [[T.seg(p, [pp(s1, p), pp(s1, p)])], [T.seg(p, [pp(s1, p)])]],
        "stale view": [[T.seg(0, [pp(s1, 0, view=0)]), T.seg(p, [pp(s1, p, view=T.VIEW + n), pp(s2, p)])]],
        "outside the window": [[T.seg(p, [pp(q, p) for q in (0, T.WINDOW, T.WINDOW + 1, 2**64 - 1)])]],
        "escaped operation": escaped,
        "between votes": between,
    }


# ---- the decoder's corpus ----
def _op(k, salt=0):
    return bytes(ALPHABET[(7 * i + salt) % len(ALPHABET)] for i in range(k))


def _msg(rng, **kw):
    from pbft_amd import wire
    d = dict(kind=0, view=7, seq=3, digest=rng.bytes(64), replica=1, sig=rng.bytes(64), operation=b"op-3", timestamp=5,
             client="127.0.0.1:8080")
    d.update(kw)
    return wire.WireMsg(**d)


def corpus():
    """[(body, inside)]: inside = made by the encoder within the stated alphabet and limits (must be PBFT_PP_OK)."""
    from pbft_amd import wire
    rng = np.random.RandomState(20240611)
    enc = wire.encode_json
    out = []
    for k in (0, 1, 111, 112, 127, 128, 129, 255, 256, 257, 3071, 3072, 3073):
        out.append((enc(_msg(rng, operation=_op(k, k))), k <= OP_MAX))
    wide = (1, 9, 10**19, 2**64 - 1)
    for v in wide:
        out.append((enc(_msg(rng, view=v)), True))
        out.append((enc(_msg(rng, seq=v)), True))
        out.append((enc(_msg(rng, timestamp=v)), True))
    out.append((enc(_msg(rng, view=0, seq=0, timestamp=0)), True))
    out.append((enc(_msg(rng, view=2**64 - 1, seq=2**64 - 1, timestamp=2**64 - 1, replica=65535)), True))
    for field in (b'"view":', b'"sequence_number":', b'"timestamp":'):  # 2^64 and a leading zero: no encoder writes them
        body = enc(_msg(rng, view=7, seq=7, timestamp=7))
        out.append((body.replace(field + b"7", field + b"18446744073709551616", 1), False))
        out.append((body.replace(field + b"7", field + b"07", 1), False))
    for r in (0, 65535):
        out.append((enc(_msg(rng, replica=r)), True))
    out.append((enc(_msg(rng, replica=7)).replace(b'"replica":7', b'"replica":65536', 1), False))
    for k in (1, 63, 64):
        out.append((enc(_msg(rng, client="c" * k)), k <= 63))
    out.append((enc(_msg(rng, operation=ESCAPED)), False))
    out.append((enc(_msg(rng, operation="café".encode())), False))
    out.append((enc(_msg(rng, operation=b"a\x7fb")), False))
    out.append((enc(_msg(rng, sig=None, replica=None)), False))  # unsigned
    for kind in (1, 2):
        out.append((enc(_msg(rng, kind=kind)), False))
        out.append((enc(_msg(rng, kind=kind, view=10**19, seq=10**19, replica=65535)), False))
    out.append((enc(_msg(rng, kind=3)), False))
    out.append((enc(_msg(rng, kind=3, operation=_op(400))), False))
    bases = [enc(_msg(rng, operation=b"")), enc(_msg(rng, operation=b"op-5")),
             enc(_msg(rng, view=10**19, operation=_op(130), client="[::1]:9"))]
    for base in bases:
        for at in range(len(base)):
            for c in b'"\\\x1f\x7f\x80 0}A':
                if base[at] != c:
                    out.append((base[:at] + bytes([c]) + base[at + 1:], False))
        for k in range(len(base)):
            out.append((base[:k], False))
        for tail in (b"}", b" ", b"\n", b"}}", b"  ", b"\x00\x00\x00"):
            out.append((base + tail, False))
        # swapped field pairs
        i_v, i_n, i_d = base.index(b'"view":'), base.index(b',"sequence_number":'), base.index(b',"digest":')
        out.append((base[:i_v] + base[i_n + 1:i_d] + b"," + base[i_v:i_n] + base[i_d:], False))
        i_m, i_r, i_s = base.index(b',"message":'), base.index(b',"replica":'), base.index(b',"signature":')
        out.append((base[:i_m] + base[i_r:i_s] + base[i_m:i_r] + base[i_s:], False))
        out.append((base[:i_r] + base[i_s:-2] + base[i_r:i_s] + b"}}", False))
        i_t, i_c = base.index(b',"timestamp":'), base.index(b',"client":')
        i_e = base.index(b'},"replica":')
        out.append((base[:i_t] + base[i_c:i_e] + base[i_t:i_c] + base[i_e:], False))
    return out


def extremes():
    """The shortest and the longest canonical frame, and one byte more."""
    from pbft_amd import wire
    rng = np.random.RandomState(7)
    big = 2**64 - 1
    lo = wire.encode_json(_msg(rng, view=0, seq=9, timestamp=1, replica=0, operation=b"", client="c"))
    hi = wire.encode_json(_msg(rng, view=big, seq=big, timestamp=big, replica=65535, operation=_op(OP_MAX),
                               client="c" * 63))
    over = wire.encode_json(_msg(rng, view=big, seq=big, timestamp=big, replica=65535, operation=_op(OP_MAX + 1),
                                 client="c" * 63))
    return lo, hi, over
