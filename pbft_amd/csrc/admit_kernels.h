// Launcher of the replica's admission pass (admit.hip): N decoded frames' heads -> class per frame, class counts, the
// clean bitmap, the residue list, and key index 0xFFFF in the record of every frame that is not clean.  Called by
// pbft_admit_device (pbft_verify.hip), which owns the workspace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "admit_core.h"

static constexpr int ADMIT_BLOCK = 256;        // 4 waves; wave w of the grid covers rows [64 w, 64 w + 64)
static constexpr int ADMIT_SCAN_BLOCK = 1024;  // the one block that prefix-sums the residue marks
static constexpr uint64_t ADMIT_MAX_ROWS = (uint64_t)1 << 31;

struct admit_residue {  // pbft_admit_residue of include/pbft_wire.h
  uint64_t off;
  uint32_t frame, len;
};

// The workspace of one call, carved from a context buffer: seen plane | twice plane (32-bit words, side by side so
// that one kernel zeroes both) | one residue mark bit per row | the marks' exclusive prefix per 64-row word.
// Monotone in both arguments: a buffer reserved for (plane_bits, max_n) holds every smaller call.
struct admit_ws {
  uint64_t plane_words, words;  // 32-bit words of ONE plane (a multiple of 4); 64-row words
  size_t off_twice, off_flags, off_prefix, total;
  admit_ws(uint64_t plane_bits, uint64_t N) {
    plane_words = ((plane_bits + 127) / 128) * 4;
    words = (N + 63) / 64;
    off_twice = (size_t)plane_words * 4;
    off_flags = (2 * off_twice + 255) & ~(size_t)255;
    off_prefix = off_flags + ((8 * (size_t)words + 255) & ~(size_t)255);
    total = off_prefix + ((4 * (size_t)words + 255) & ~(size_t)255);
  }
};

// Five kernel launches on st (zero, mark, resolve, scan, emit); no allocation, copy, memset or synchronisation.
// ws holds admit_ws(admit_plane_bits(log_window, n_keys), N).total bytes, 256-byte aligned.  n_frames: null (every
// row is a frame) or the index's {total, not written}, read on the device.  N <= ADMIT_MAX_ROWS; N = 0 writes zero
// counts, n_res = {0, 0} and zeroes res[residue_cap].
hipError_t launch_admit(const pbft::admit_head* heads, uint8_t* records, const uint64_t* off, const uint32_t* len,
                        const uint32_t* n_frames, uint64_t N, uint64_t view, uint64_t h, uint64_t log_window,
                        uint32_t n_keys, uint32_t residue_cap, uint8_t* ws, uint8_t* cls, uint32_t* counts,
                        uint64_t* clean, admit_residue* res, uint32_t* n_res, hipStream_t st);
