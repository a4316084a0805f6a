// TEST INFRASTRUCTURE: the arithmetic op table of pbft_amd/csrc/debug_arith_core.h compiled for the HOST -- the same
// debug_arith_item the library's pbft_debug_arith runs on the GPU, looped over n items, with the same arguments
// and error convention (tests/test_arith.py).  Its own small library beside host_harness.cpp; never loaded by the
// product path.
#include "../../pbft_amd/csrc/debug_arith_core.h"

using namespace pbft;

extern "C" int hh_arith_info(int op, const char** name, uint32_t* win, uint32_t* wout) {
  const debug_arith_desc* d = debug_arith_lookup(op);
  if (!d) return -1;
  if (name) *name = d->name;
  if (win) *win = d->win;
  if (wout) *wout = d->wout;
  return 0;
}

extern "C" int hh_arith(int op, const uint32_t* in, uint32_t* out, uint32_t n) {
  const debug_arith_desc* d = debug_arith_lookup(op);
  if (!in || !out || !d || n == 0 || n > (1u << 20)) return -1;
  for (uint32_t i = 0; i < n; ++i) debug_arith_item(op, in + (size_t)i * d->win, out + (size_t)i * d->wout);
  return 0;
}
