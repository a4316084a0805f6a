// Launchers of the client-reply kernels (reply.hip): N executed requests -> the digests D = Blake2b-512(C | result), this
// replica's signatures over the kind-3 envelopes, and the canonical replies' signed texts with their offsets.  Called by
// pbft_sign_replies_device (pbft_verify.hip), which owns the key buffer (egress_kernels.h) and the workspace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "egress_kernels.h"
#include "reply_core.h"

static constexpr uint32_t REPLY_TILE = 64;  // replies per scan tile: one wave
// The PeerId text of the installed identity (52 characters, 13 words) in the free words of the signer's state
// (egress_kernels.h: words 0 .. 24 the key, 24 the replica index, 32 .. 39 the seed's staging area); written by
// pbft_sign_set_seed from the public key that came back: there is no base58 on the device.
static constexpr uint32_t REPLY_KEY_PEER_ID = 40;
static_assert(REPLY_KEY_PEER_ID >= EGRESS_KEY_SEED + 8 && 4 * (EGRESS_KEY_WORDS - REPLY_KEY_PEER_ID) >= pbft::RP_PEER_ID_B58,
              "the text fits behind the seed's staging area");
// the workspace of one call: one u64 per tile (its texts' bytes, then the bytes in front of it)
static inline size_t reply_ws_bytes(uint64_t N) {
  return (8 * (size_t)((N + REPLY_TILE - 1) / REPLY_TILE) + 255) & ~(size_t)255;
}

// Three kernel launches on st (the canonical test, lengths and their scan inside each tile; the scan over the tiles;
// digest, signature and texts); no allocation, copy, memset or synchronisation.  N <= RP_MAX_N; N = 0 writes
// reply_off[0] = 0 with one launch.  ws holds reply_ws_bytes(N) bytes, 8-byte aligned.  d_key: the signer's state as
// launch_egress_seed wrote it, with the PeerId text at word REPLY_KEY_PEER_ID.
hipError_t launch_reply(const uint8_t* d_results, uint64_t results_bytes, const uint64_t* d_res_off,
                        const uint32_t* d_res_len, const uint64_t* d_timestamp, const uint8_t* d_clients, uint64_t view,
                        uint64_t N, const uint32_t* d_key, const uint32_t* tabB, uint64_t* ws, uint8_t* d_out,
                        uint64_t out_cap, uint64_t* d_reply_off, uint8_t* d_digests, uint8_t* d_sigs, uint8_t* d_status,
                        hipStream_t st);
