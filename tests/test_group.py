"""Envelope grouping without a GPU: group_reference (the numpy statement of pbft_group_envelopes_device) on
hand-written cases, and the new entry points' presence and arity in the headers, the ctypes table and pbft-hip's
ffi.rs."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_crate import _header_decls, _rust_decls

NONE = 0xFFFFFFFF
NEW = {"pbft_group_envelopes_device": 11, "pbft_group_reserve": 2, "pbft_verify_frames_tally_device": 18,
       "pbft_verify_frames_tally": 16}


def env(kind, view, seq, fill):
    """An 85-byte envelope: "PBFT", kind, view, seq (little endian), a digest of one repeated byte."""
    e = np.zeros(85, np.uint8)
    e[:4] = np.frombuffer(b"PBFT", np.uint8)
    e[4] = kind
    e[5:13] = np.frombuffer(int(view).to_bytes(8, "little"), np.uint8)
    e[13:21] = np.frombuffer(int(seq).to_bytes(8, "little"), np.uint8)
    e[21:] = fill
    return e


def test_first_appearance_order():
    from pbft_amd import group_reference
    a, b, c = env(1, 0, 7, 0x11), env(1, 0, 8, 0x22), env(1, 0, 9, 0x33)
    rows = np.stack([b, a, b, c, a, a, c])
    idx, table, n = group_reference(rows, None, 5)
    assert idx.dtype == np.uint32 and idx.tolist() == [0, 1, 0, 2, 1, 1, 2]
    assert table.shape == (5, 85) and (table[0] == b).all() and (table[1] == a).all() and (table[2] == c).all()
    assert not table[3:].any() and n.dtype == np.uint32 and n.tolist() == [3, 0]


def test_rows_wider_than_an_envelope_use_their_first_85_bytes():
    from pbft_amd import group_reference
    rows = np.zeros((4, 96), np.uint8)
    rows[:, :85] = np.stack([env(1, 1, 1, 5), env(1, 1, 1, 5), env(1, 1, 2, 5), env(1, 1, 1, 5)])
    rows[:, 85:] = np.arange(44, dtype=np.uint8).reshape(4, 11)  # what follows the envelope is not part of the key
    idx, table, n = group_reference(rows, None, 2)
    assert idx.tolist() == [0, 0, 1, 0] and n.tolist() == [2, 0] and (table[1] == rows[2, :85]).all()


def test_skipped_rows_take_part_in_nothing():
    from pbft_amd import group_reference
    a, b, c = env(2, 3, 1, 1), env(2, 3, 2, 2), env(2, 3, 3, 3)
    rows = np.stack([c, a, b, c, a])
    skip = np.array([True, False, False, False, True])  # row 0's envelope first appears, unskipped, at row 3
    idx, table, n = group_reference(rows, skip, 4)
    assert idx.tolist() == [NONE, 0, 1, 2, NONE]
    assert (table[0] == a).all() and (table[1] == b).all() and (table[2] == c).all() and not table[3].any()
    assert n.tolist() == [3, 0]
    idx, table, n = group_reference(rows, np.ones(5, bool), 4)  # every row skipped: no envelope
    assert (idx == NONE).all() and not table.any() and n.tolist() == [0, 0]


def test_overflow_accounting():
    from pbft_amd import group_reference
    e = [env(1, 0, s, s) for s in range(4)]
    rows = np.stack([e[0], e[1], e[2], e[1], e[3], e[2], e[0], e[3], e[3]])
    idx, table, n = group_reference(rows, None, 2)
    assert idx.tolist() == [0, 1, NONE, 1, NONE, NONE, 0, NONE, NONE]
    assert n.tolist() == [4, 5]  # four distinct envelopes found, five rows left without an index
    assert (table[0] == e[0]).all() and (table[1] == e[1]).all() and table.shape == (2, 85)
    idx, table, n = group_reference(rows, None, 1)
    assert idx.tolist() == [0, NONE, NONE, NONE, NONE, NONE, 0, NONE, NONE] and n.tolist() == [4, 7]
    idx, table, n = group_reference(rows, None, 4)
    assert idx.tolist() == [0, 1, 2, 1, 3, 2, 0, 3, 3] and n.tolist() == [4, 0]
    with pytest.raises(ValueError):
        group_reference(rows, None, 0)
    idx, table, n = group_reference(np.zeros((0, 85), np.uint8), None, 0)  # no rows: nothing, whatever the capacity
    assert len(idx) == 0 and table.shape == (0, 85) and n.tolist() == [0, 0]


def test_prepare_and_commit_are_two_envelopes_and_every_byte_counts():
    from pbft_amd import group_reference
    p, c = env(1, 4, 9, 0xAB), env(2, 4, 9, 0xAB)
    first, last = p.copy(), p.copy()
    first[21] ^= 1  # the digest's first byte
    last[84] ^= 0x80  # the envelope's last byte
    rows = np.stack([p, c, first, last, c, p, last])
    idx, table, n = group_reference(rows, None, 8)
    assert idx.tolist() == [0, 1, 2, 3, 1, 0, 3] and n.tolist() == [4, 0]
    assert table[0, 4] == 1 and table[1, 4] == 2 and (table[0, 5:] == table[1, 5:]).all()


def test_header_declares_the_new_entry_points():
    h = _header_decls()
    for name, arity in NEW.items():
        assert h.get(name) == arity, (name, h.get(name))
    src = open(os.path.join(ROOT, "include", "pbft_verify.h")).read()
    assert re.search(r"#define PBFT_OPT_GROUP_SEED 16\b", src) and re.search(r"#define PBFT_OPT_GROUP_HASH_BITS 17\b", src)


def test_ctypes_table_binds_the_new_entry_points():
    import pbft_amd
    lib = pbft_amd.load()
    for name, arity in NEW.items():
        assert name in pbft_amd.EXPORTS, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == arity, (name, fn.argtypes)
    v = pbft_amd.GpuBatchVerifier
    assert (v.OPT_GROUP_SEED, v.OPT_GROUP_HASH_BITS) == (16, 17)
    for method in ("group_envelopes_device", "group_reserve", "verify_frames_tally_device", "verify_frames_tally"):
        assert callable(getattr(v, method)), method
    # null arguments are errors, not crashes
    assert lib.pbft_group_envelopes_device(None, None, 85, None, 2, 0, 0, None, None, None, None) == -1
    assert lib.pbft_group_reserve(None, 0) == -1
    assert lib.pbft_verify_frames_tally(None, None, 0, None, None, None, 4, 0, 0, None, None, None, None, None, None,
                                        None) == -1


def test_ffi_rs_binds_the_new_entry_points():
    r = _rust_decls()
    for name, arity in NEW.items():
        assert r.get(name) == arity, (name, r.get(name))
    lib = open(os.path.join(ROOT, "pbft-hip", "src", "lib.rs")).read()
    assert "pub fn verify_frames_tally(" in lib and "pub struct FramesTally" in lib
    assert "ffi::pbft_verify_frames_tally(" in lib
