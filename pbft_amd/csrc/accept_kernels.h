// Launchers of the client-acceptance kernels (accept.hip): N signed replies' texts -> verifier records and heads; and,
// behind grouping, verification and tally, one certificate per envelope.  Called by pbft_wire_decode_replies_device,
// pbft_accept_replies_device and pbft_accept_replies (pbft_verify.hip), which own the PeerId table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "accept_core.h"

static constexpr uint32_t ACCEPT_TILE = 64;  // replies per tile: one wave, one workgroup

// One kernel node on st: reply i = bytes [d_off[i], d_off[i] + d_len[i]) of d_text -> d_records[i] (160 bytes) and
// d_heads[i] (32 bytes).  d_text is 16-byte aligned; only aligned dwords that hold a byte of a reply inside text_bytes
// are read.  d_client_idx: null (every reply is client 0) or one index per reply; d_clients: [n_clients][64];
// d_pid: [n_keys][52].  N > 0.
hipError_t launch_accept_decode(const uint8_t* d_text, uint64_t text_bytes, const uint64_t* d_off, const uint32_t* d_len,
                                const uint32_t* d_client_idx, const uint8_t* d_clients, uint32_t n_clients,
                                const uint8_t* d_pid, uint32_t n_keys, uint64_t N, uint8_t* d_records, void* d_heads,
                                hipStream_t st);

// Three kernel nodes on st: every certificate of [0, env_cap) initialised (zero, first = 0xFFFFFFFF); the least valid
// reply of each envelope by atomicMin; view, timestamp, count, client and accepted of the envelopes below
// min(d_n_env[0], env_cap).  env_cap > 0.
hipError_t launch_accept_certify(const uint64_t* d_bitmap, const uint32_t* d_env_idx, const uint32_t* d_client_idx,
                                 uint64_t N, const uint8_t* d_envelopes, const uint32_t* d_n_env,
                                 const uint32_t* d_count, uint32_t env_cap, uint32_t need, void* d_certs,
                                 hipStream_t st);

// P settled replies scattered into the N records and heads: idx [P], prec [P][160], phead [P][32].
hipError_t launch_accept_patch(const uint32_t* d_idx, const uint8_t* d_prec, const void* d_phead, uint32_t P, uint64_t N,
                               uint8_t* d_records, void* d_heads, hipStream_t st);
