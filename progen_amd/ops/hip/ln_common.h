// What the LN + token-shift kernels share, forward and backward
// (ln_shift.hip, ln_shift_bwd_body.h, bias_grad.hip): the block size, the
// table of a kernel template's eight instantiations, and the block sum.
#pragma once

#include "common.h"

#define LN_BLOCK 256
#define LN_WAVES (LN_BLOCK / WAVE)

// the eight instantiations of a kernel template on three bools, indexed by
// the bools as bits 2, 1, 0
#define LN_KERNEL(K, i) K<((i) & 4) != 0, ((i) & 2) != 0, ((i) & 1) != 0>
#define LN_TABLE(K)                                                     \
  {LN_KERNEL(K, 0), LN_KERNEL(K, 1), LN_KERNEL(K, 2), LN_KERNEL(K, 3), \
   LN_KERNEL(K, 4), LN_KERNEL(K, 5), LN_KERNEL(K, 6), LN_KERNEL(K, 7)}

// sum over the block, result in every thread, through a LN_WAVES-float
// shared scratch (all threads must reach this together): per-wave sums,
// then an xor-shuffle tree over the wave partials in wave 0. The trailing
// barrier frees ``red`` for the next call.
__device__ __forceinline__ float ln_block_sum(float a, float* red) {
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  a = wave_sum(a);
  if (lane == 0) red[wid] = a;
  __syncthreads();
  if (wid == 0) {
    float t = (lane < LN_WAVES) ? red[lane] : 0.f;
#pragma unroll
    for (int off = LN_WAVES / 2; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
    if (lane == 0) red[0] = t;
  }
  __syncthreads();
  a = red[0];
  __syncthreads();
  return a;
}
