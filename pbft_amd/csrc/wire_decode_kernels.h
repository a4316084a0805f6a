// Launchers of the frame decoder (wire_decode.hip): signed-vote JSON frames -> 160-byte records and 24-byte heads.
// Called by pbft_wire_decode_frames_device and the host form pbft_verify_frames (pbft_verify.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

static constexpr int FRAMES_BLOCK = 64;  // one wave per block: frame 64 b + lane; 25,600 B of LDS

// Frame f = bytes [off[f], off[f] + len[f]) of d_stream -> records[f] (160 B) and heads[f] (24 B).  d_stream is
// 16-byte aligned and readable up to stream_bytes rounded up to 16; records 16-byte, heads 8-byte aligned.  N > 0.
hipError_t launch_decode_frames(const uint8_t* d_stream, uint64_t stream_bytes, const uint64_t* d_off,
                                const uint32_t* d_len, const uint16_t* d_peer, uint32_t n_replicas, uint64_t N,
                                uint8_t* d_records, void* d_heads, hipStream_t st);
// records[idx[p]] = prec[p], heads[idx[p]] = phead[p] for p < P (idx[p] >= N is skipped): the frames the host parser
// settled.  prec 16-byte, phead 8-byte aligned.  P > 0.
hipError_t launch_patch_frames(const uint32_t* d_idx, const uint8_t* d_prec, const void* d_phead, uint32_t P,
                               uint64_t N, uint8_t* d_records, void* d_heads, hipStream_t st);
