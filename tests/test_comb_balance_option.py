"""PBFT_OPT_COMB_BALANCE has one number in the C header, the Python binding and the Rust crate, and the library's
option switch handles it (no GPU needed)."""
import os
import re

from conftest import ROOT


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def test_option_number_is_mirrored():
    hdr = _read("include", "pbft_verify.h")
    m = re.search(r"#define PBFT_OPT_COMB_BALANCE (\d+)\b", hdr)
    assert m
    num = int(m.group(1))
    others = [int(x) for x in re.findall(r"#define PBFT_OPT_\w+ (\d+)\b", hdr)]
    assert others.count(num) == 1  # no other option has this number
    assert re.search(rf"OPT_COMB_BALANCE = {num}\b", _read("pbft_amd", "verifier.py"))
    assert re.search(rf"pub const PBFT_OPT_COMB_BALANCE: c_int = {num};", _read("pbft-hip", "src", "ffi.rs"))
    assert "case PBFT_OPT_COMB_BALANCE:" in _read("pbft_amd", "csrc", "pbft_verify.hip")
