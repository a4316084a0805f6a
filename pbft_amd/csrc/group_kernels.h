// Launcher of the envelope grouping (group.hip): N rows' 85-byte envelopes -> env_idx per row, the table of distinct
// envelopes in order of first appearance, and their number.  Called by pbft_group_envelopes_device (pbft_verify.hip),
// which owns the workspace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

static constexpr int GROUP_BLOCK = 256;            // 4 waves; wave w of the grid covers rows [64 w, 64 w + 64)
static constexpr int GROUP_SCAN_BLOCK = 1024;      // the one block that prefix-sums the representative marks
static constexpr uint32_t GROUP_NONE = 0xFFFFFFFFu;  // an empty slot; a row without an envelope index
static constexpr uint32_t GROUP_ENV_BYTES = 85;
static constexpr uint64_t GROUP_MAX_ROWS = (uint64_t)1 << 31;

// Slots of the open-addressing table for N rows: a power of two >= 2 N (>= 64), so an empty slot always exists.
static inline uint64_t group_table_slots(uint64_t N) {
  uint64_t t = 64;
  while (t < 2 * N) t <<= 1;
  return t;
}

// The workspace of one call, carved from a context buffer: table | slot of each row | one mark bit per row | the
// marks' exclusive prefix per 64-row word.  group_ws_bytes is monotone in N: a buffer reserved for max_n holds
// every N <= max_n.
struct group_ws {
  uint64_t slots, words;
  size_t off_slot, off_flags, off_prefix, total;
  explicit group_ws(uint64_t N) {
    slots = group_table_slots(N);
    words = (N + 63) / 64;
    off_slot = (size_t)slots * 4;
    off_flags = off_slot + ((4 * (size_t)N + 255) & ~(size_t)255);
    off_prefix = off_flags + ((8 * (size_t)words + 255) & ~(size_t)255);
    total = off_prefix + ((4 * (size_t)words + 255) & ~(size_t)255);
  }
};
static inline size_t group_ws_bytes(uint64_t N) { return group_ws(N).total; }

// Five kernel launches on st (fill, insert, mark, scan, assign); no allocation, copy, memset or synchronisation.
// msg / key are byte pointers to row 0's envelope and key index (key: null = no row is skipped), each read with
// its byte stride; ws holds group_ws_bytes(N) bytes, 256-byte aligned.  N <= GROUP_MAX_ROWS; N = 0 writes
// n_env = {0, 0} and zeroes envelopes[env_cap][85].  hash_bits <= 64.
hipError_t launch_group(const uint8_t* msg, uint32_t msg_stride, const uint8_t* key, uint32_t key_stride, uint64_t N,
                        uint32_t env_cap, uint64_t seed, uint32_t hash_bits, uint8_t* ws, uint32_t* env_idx,
                        uint8_t* envelopes, uint32_t* n_env, hipStream_t st);
