// Decode-step prologue on one row per batch element: residual add,
// scale-only LayerNorm and the token shift (the decode analogue of
// ln_shift.hip's RES variant).
//
//   h    <- h + res            (stored in the tensor dtype; skipped without res)
//   ln    = LN(h) * g          (statistics in fp32, from h AS STORED)
//   y     = [prev[:D/2] | ln[D/2:]]   if shift, else ln
//   prev <- ln                 (whole row; skipped without prev)
//
// One 256-thread workgroup per row; a thread owns 8-element chunks
// tid, tid + 256, ... and reads its prev chunk before overwriting it, so
// no thread ever reads what another one writes. Rows up to 2048 wide
// (ONE) keep their single chunk in registers across the three passes;
// wider rows re-read h, which by then holds the summed stream. The body is
// in decode_ln_shift_body.h, shared with the slot kernel.

#include "common.h"
#include "decode_kernels.h"
#include "decode_ln_shift_body.h"

template <bool BF, bool ONE>
__global__ __launch_bounds__(256) void dec_ln_shift_kernel(
    void* h, const void* __restrict__ res, const void* __restrict__ g,
    void* prev, void* __restrict__ y, int D, float eps, bool shift) {
  dec_ln_shift_body<BF, ONE, false>(h, res, g, prev, y, nullptr, D, eps,
                                    shift);
}

extern "C" hipError_t dec_ln_shift_launch(void* h, const void* res,
                                          const void* g, void* prev, void* y,
                                          int B, int D, float eps, bool shift,
                                          bool is_bf16, hipStream_t stream) {
#define GO(BF, ONE)                                                   \
  dec_ln_shift_kernel<BF, ONE><<<B, 256, 0, stream>>>(h, res, g, prev, y, D, \
                                                      eps, shift)
  const bool one = D <= 2048;
  if (is_bf16) {
    if (one) GO(true, true); else GO(true, false);
  } else {
    if (one) GO(false, true); else GO(false, false);
  }
#undef GO
  return hipGetLastError();
}
