// The canonical-PrePrepare rule (pbft_amd/csrc/wire_pp_core.h) built for the host as a stand-alone program, for
// AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_pp.py).  Reads frames from a file (u32 count, then per
// frame u32 length and the bytes), runs the core and the digest over each frame in a heap buffer of exactly its length
// -- a read of one byte outside the frame is a sanitizer report -- and writes one 232-byte pbft_pp_head per frame.
//   pp_main <frames file> <heads file>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/pbft_wire.h"
#include "../../pbft_amd/csrc/wire_pp_core.h"

using namespace pbft;

static_assert(PP_FRAME_MIN == PBFT_PP_FRAME_MIN && PP_FRAME_MAX == PBFT_PP_FRAME_MAX && PP_OP_MAX == PBFT_PP_OP_MAX, "");

static void decode(const uint8_t* body, uint32_t len, pbft_pp_head* out) {
  memset(out, 0, sizeof *out);
  const frame_mem_reader rd{body, 0, len, 0xAA};
  pp_fields h;
  if (wire_pp_frame(rd, pp_byte_scan<frame_mem_reader>{rd}, 0, len, h) != PP_ST_OK) return;
  out->view = h.view;
  out->seq = h.seq;
  out->timestamp = h.timestamp;
  out->op_off = h.op_off;
  out->op_len = h.op_len;
  out->replica = (uint16_t)h.replica;
  out->status = PBFT_PP_OK;
  memcpy(out->claimed, h.claimed, 64);
  memcpy(out->sig, h.sig, 64);
  pp_digest(out->computed, body, h.op_off, h.op_len);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  uint32_t n = 0;
  if (fread(&n, 4, 1, in) != 1) return 2;
  uint64_t ok = 0;
  for (uint32_t f = 0; f < n; ++f) {
    uint32_t len = 0;
    if (fread(&len, 4, 1, in) != 1) return 2;
    uint8_t* body = (uint8_t*)malloc(len ? len : 1);  // exactly the frame (a zero-length one gets a byte nobody reads)
    if (len && fread(body, 1, len, in) != len) return 2;
    pbft_pp_head h;
    decode(body, len, &h);
    ok += h.status == PBFT_PP_OK;
    free(body);
    if (fwrite(&h, sizeof h, 1, out) != 1) return 2;
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  printf("pp host run ok: %u frames, %llu accepted\n", n, (unsigned long long)ok);
  return 0;
}
