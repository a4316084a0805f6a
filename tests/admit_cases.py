"""Cases of the replica's admission pass, shared by tests/test_admit.py (host build of admit_core.h against
pbft_amd.admit_reference) and tests/test_gpu_admit.py (pbft_admit_device against the same reference).  A case is a
list of rows (status, kind, view, seq, key_idx) -- a decoded frame's head -- plus the replica's (view, h, log_window),
n_keys, residue_cap and n_total (None: every row is a frame)."""
import numpy as np

from pbft_amd.wire import FrameHead

VIEW = 1
OK, ESIGNER, EDEFER = 0, 5, 6
M64 = (1 << 64) - 1


def vote(kind, seq, key, view=VIEW, status=OK):
    return (status, kind, view, seq & M64, key)


def not_ok(status):
    """What the frame decoder writes for a frame that is not PBFT_WIRE_OK."""
    return (status, 0, 0, 0, 0xFFFF)


def case(name, rows, h=0, log_window=64, n_keys=16, residue_cap=None, n_total=None, view=VIEW):
    return dict(name=name, rows=list(rows), view=view, h=h, log_window=log_window, n_keys=n_keys,
                residue_cap=len(rows) + 3 if residue_cap is None else residue_cap, n_total=n_total)


def distinct_votes(n, log_window=64, n_keys=16, h=0):
    """n admitted votes with pairwise distinct (kind, seq, signer); n <= 2 * log_window * n_keys."""
    assert n <= 2 * log_window * n_keys
    return [vote(1 + (i // n_keys) % 2, h + 1 + i // (2 * n_keys), i % n_keys) for i in range(n)]


def contested(groups, n=300):
    """Distinct votes in which every group of rows shares the (kind, seq, signer) of the group's first row."""
    rows = distinct_votes(n)
    for g in groups:
        for i in g[1:]:
            rows[i] = rows[g[0]]
    return rows


def random_rows(n, seed, h=7, log_window=16, n_keys=7):
    """A mixture: mostly admitted votes drawn from few keys (so that many are contested), the rest every other class."""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        x = rng.integers(0, 20)
        kind, key = int(rng.integers(1, 3)), int(rng.integers(0, n_keys))
        seq = h + 1 + int(rng.integers(0, log_window))
        if x < 12:
            rows.append(vote(kind, seq, key))
        elif x == 12:
            rows.append(vote(kind, seq, key, view=VIEW + 1))
        elif x == 13:
            rows.append(vote(kind, h - int(rng.integers(0, 3)), key))
        elif x == 14:
            rows.append(vote(kind, h + log_window + 1 + int(rng.integers(0, 3)), key))
        elif x == 15:
            rows.append(not_ok(ESIGNER))
        elif x == 16:
            rows.append(vote(0, seq, key))
        else:
            rows.append(not_ok(EDEFER))
    return rows


def cases():
    hw = (1 << 64) - 3
    out = [
        case("watermarks", [vote(k, s, k) for k in (1, 2) for s in (10, 11, 18, 19)], h=10, log_window=8, n_keys=4),
        case("window past 2^64", [vote(1, s, i % 4) for i, s in enumerate(
            (hw, hw + 1, hw + 2, hw + 3, hw + 4, hw + 8, hw + 9, 5, hw - 1))], h=hw, log_window=8, n_keys=4),
        case("view before window", [vote(1, 999, 0, view=VIEW + 1), vote(2, 0, 1, view=0), vote(1, 3, 2, view=VIEW + 1),
                                    vote(1, 999, 3)], h=0, log_window=8, n_keys=4),
        case("every status", [not_ok(s) for s in range(1, 8)] + [not_ok(255)] +
             [vote(1, 3, 1, status=s) for s in range(0, 8)] + [vote(0, 3, 2), vote(3, 3, 2), vote(2, 3, 2),
                                                               vote(1, 4, 16), vote(1, 4, 0xFFFF), vote(1, 4, 15)]),
        case("both kinds", [vote(1, 5, 3), vote(2, 5, 3), vote(1, 6, 3), vote(2, 5, 4)]),
        case("pairs", contested([(0, 1), (63, 64), (255, 256)])),
        case("triples", contested([(0, 1, 299), (63, 64, 130), (255, 256, 2)])),
        case("pairs across kinds", contested([(0, 1)], n=16) + [vote(2, 1, 0)]),
        case("padding", distinct_votes(70) + [not_ok(EDEFER)] * 3, n_total=66),
        case("total above N", distinct_votes(10) + [not_ok(EDEFER)], n_total=1000),
        case("nothing valid", distinct_votes(5), n_total=0),
        case("residue cap", contested([(0, 1), (63, 64)], n=130) + [not_ok(EDEFER)] * 5, residue_cap=3),
        case("no residue room", contested([(0, 1)], n=10), residue_cap=0),
        case("largest window", [vote(1, 1, 0), vote(2, 1 << 14, (1 << 15) - 1), vote(2, 1 << 14, (1 << 15) - 1),
                                vote(1, (1 << 14) + 1, 0)], log_window=1 << 14, n_keys=1 << 15),
    ]
    for n in (1, 63, 64, 65, 4099):
        out.append(case(f"random {n}", random_rows(n, 1000 + n), h=7, log_window=16, n_keys=7,
                        residue_cap=max(1, n // 3)))
    return out


def to_heads(rows):
    heads = np.zeros(len(rows), dtype=FrameHead)
    for i, (status, kind, view, seq, key) in enumerate(rows):
        heads[i] = (view, seq, key, kind, status, 340 + i % 40)
    return heads


def index_of(n):
    """A stand-in frame index: off / len of n frames."""
    return (1000 + 400 * np.arange(n, dtype=np.uint64)), (340 + np.arange(n, dtype=np.uint32) % 40).astype(np.uint32)


def permute_in_waves(rows, seed):
    """The same rows, shuffled inside every run of 64."""
    rng = np.random.default_rng(seed)
    perm = np.concatenate([lo + rng.permutation(min(64, len(rows) - lo)) for lo in range(0, len(rows), 64)]) \
        if rows else np.zeros(0, np.int64)
    return [rows[i] for i in perm], perm
