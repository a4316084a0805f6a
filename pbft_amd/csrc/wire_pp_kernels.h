// Launcher of the PrePrepare kernels (wire_pp.hip): the residue of the admission pass -> one pbft_pp_head per entry.
// Called by pbft_wire_decode_preprepares_device and pbft_verify_streams_admit_pp (pbft_verify.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Entry i < n_entries of d_res (pbft_admit_residue) -> d_pp[i] (pbft_pp_head): parsed by pp_parse_kernel, `computed`
// filled in by pp_digest_kernel.  d_n_res: NULL, or the live count (entries from min(d_n_res[0], n_entries) on are
// zeroed).  d_stream is 16-byte aligned and readable up to stream_bytes rounded up to 16; d_res and d_pp 8-byte
// aligned.  n_entries > 0.  Two kernel nodes, nothing else.
hipError_t launch_pp(const uint8_t* d_stream, uint64_t stream_bytes, const void* d_res, const uint32_t* d_n_res,
                     uint32_t n_entries, void* d_pp, hipStream_t st);
