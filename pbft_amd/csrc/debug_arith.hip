// Test hook: the field, scalar and comb-step arithmetic as compiled for gfx950, on raw words (debug_arith_core.h).
// Its own translation unit; nothing on the verify path calls it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "debug_arith_core.h"

using namespace pbft;

// One item per lane; lanes past n do nothing.  This kernel holds its OWN instance of fe_mul_chain, ge_madd_ab and
// the rest: it tests the source as the device compiler sees it -- the operand numbering and constraints of
// mad_column10's asm block, its FIRST and carry-in variants, dbl32, lane_mask, the bit-selects, the device form of
// sc_reduce512_fold -- and not the register allocation or schedule of comb_kernel's instance.  The round tests
// (tests/test_gpu_verify.py and the rest) remain the check of the kernels as compiled.
__global__ void __launch_bounds__(64) debug_arith_kernel(int op, const uint32_t* __restrict__ in,
                                                         uint32_t* __restrict__ out, uint32_t n, uint32_t win,
                                                         uint32_t wout) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  debug_arith_item(op, in + (size_t)i * win, out + (size_t)i * wout);
}

// name (static string) and item widths in words of op; -1 for an unknown op.  Any of the pointers may be null.
extern "C" int pbft_debug_arith_info(int op, const char** name, uint32_t* win, uint32_t* wout) {
  const debug_arith_desc* d = debug_arith_lookup(op);
  if (!d) return -1;
  if (name) *name = d->name;
  if (win) *win = d->win;
  if (wout) *wout = d->wout;
  return 0;
}

// in: n items of win words, out: n items of wout words (pbft_debug_arith_info), host memory.  Not declared in
// include/: a test hook, like pbft_debug_invert.
extern "C" int pbft_debug_arith(int op, const uint32_t* in, uint32_t* out, uint32_t n) {
  const debug_arith_desc* d = debug_arith_lookup(op);
  if (!in || !out || !d || n == 0 || n > (1u << 20)) return -1;
  uint32_t *din = nullptr, *dout = nullptr;
  const size_t bin = (size_t)n * d->win * 4, bout = (size_t)n * d->wout * 4;
  hipError_t e = hipMalloc(&din, bin);
  if (e == hipSuccess) e = hipMalloc(&dout, bout);
  if (e == hipSuccess) e = hipMemcpy(din, in, bin, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(debug_arith_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, op, din, dout, n, d->win, d->wout);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, bout, hipMemcpyDeviceToHost);
  if (din) (void)hipFree(din);
  if (dout) (void)hipFree(dout);
  return e == hipSuccess ? 0 : -(int)e - 1;
}
