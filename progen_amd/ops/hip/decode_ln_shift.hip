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
// wider rows re-read h, which by then holds the summed stream.

#include "common.h"
#include "decode_kernels.h"

template <bool BF, bool ONE>
__global__ __launch_bounds__(256) void dec_ln_shift_kernel(
    void* h, const void* __restrict__ res, const void* __restrict__ g,
    void* prev, void* __restrict__ y, int D, float eps, bool shift) {
  __shared__ float red_a[4], red_b[4];
  const long long row = (long long)blockIdx.x * D;
  const int nchunk = D >> 3;
  const int split = D >> 1;
  const int tid = threadIdx.x;
  float x[8];

  float s = 0.f;
  for (int c = tid; c < nchunk; c += 256) {
    ld8<BF>(h, row + c * 8, x);
    if (res) {
      float r[8];
      ld8<BF>(res, row + c * 8, r);
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = round_trip<BF>(x[j] + r[j]);
      st8<BF>(h, row + c * 8, x);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) s += x[j];
  }
  const float mu = block256_sum(s, red_a) / D;

  float ss = 0.f;
  for (int c = tid; c < nchunk; c += 256) {
    if (!ONE) ld8<BF>(h, row + c * 8, x);
#pragma unroll
    for (int j = 0; j < 8; ++j) ss += (x[j] - mu) * (x[j] - mu);
  }
  const float rs = rsqrtf(block256_sum(ss, red_b) / D + eps);

  for (int c = tid; c < nchunk; c += 256) {
    if (!ONE) ld8<BF>(h, row + c * 8, x);
    float gv[8], ln[8];
    ld8<BF>(g, c * 8, gv);
#pragma unroll
    for (int j = 0; j < 8; ++j) ln[j] = (x[j] - mu) * rs * gv[j];
    if (shift && c * 8 < split) {
      float pv[8];
      ld8<BF>(prev, row + c * 8, pv);
      st8<BF>(y, row + c * 8, pv);
    } else {
      st8<BF>(y, row + c * 8, ln);
    }
    if (prev) st8<BF>(prev, row + c * 8, ln);
  }
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
