"""pbft_amd — MI355X-native batch Ed25519 verifier for PBFT prepare/commit quorums.

The product is the HIP/C++ library pbft_amd/libpbft_verify.so (C ABI in
include/pbft_verify.h).  This package is the thin host-side binding used by
tests and bench.py; it never computes a signature check itself.
"""
from ._lib import EXPORTS, LIB_PATH, PbftError, load  # noqa: F401
from .verifier import (ENV_NONE, TALLY_ACCUMULATE, GpuBatchVerifier, MultiGpu, SigBatch,  # noqa: F401
                       accept_reference, admit_reference, bitmap_to_bool, group_reference, quorum, tally_reference, verify_multi)
from .wire import (AcceptCert, AcceptHead, AdmitResidue, FrameHead, PpHead, SegHead, decode_preprepare,  # noqa: F401
                   decode_reply_json, frame_index, pack_replies)

__all__ = ["GpuBatchVerifier", "MultiGpu", "SigBatch", "bitmap_to_bool", "verify_multi", "tally_reference", "quorum",
           "group_reference", "ENV_NONE", "TALLY_ACCUMULATE", "FrameHead", "SegHead", "AdmitResidue", "PpHead", "decode_preprepare", "admit_reference", "frame_index", "AcceptHead", "AcceptCert", "accept_reference", "pack_replies",
           "decode_reply_json", "PbftError", "load", "LIB_PATH",
           "EXPORTS"]
