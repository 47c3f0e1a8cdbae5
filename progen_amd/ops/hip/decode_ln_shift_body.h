// Body of the decode-step prologue (decode_ln_shift.hip), written once for
// the scalar kernel and for the slot kernel (decode_slots.hip).
//
// SLOTS = false: every row runs, ``pos`` is not read.
// SLOTS = true:  row b reads pos[b]. pos[b] < 0 is an idle row: its y row is
//                written as zeros and h and prev are not touched. pos[b] == 0
//                starts a request in a slot whose prev row still belongs to
//                the one before it, so the shifted half is zeros, not prev.
//
// The scalar and the slot kernel must give the same bits, so no fused
// multiply-add is left to the compiler: it contracts a product and a sum only
// where both land in one basic block, and which ones do differs between the
// two instantiations. Contraction is off in this body; as compiled it has
// never had an fma of its own (the variance sum is a product and an add).
#pragma once

#include "common.h"

template <bool BF, bool ONE, bool SLOTS>
__device__ __forceinline__ void dec_ln_shift_body(
    void* h, const void* __restrict__ res, const void* __restrict__ g,
    void* prev, void* __restrict__ y, const long long* __restrict__ pos, int D,
    float eps, bool shift) {
#pragma clang fp contract(off)
  __shared__ float red_a[4], red_b[4];
  const long long row = (long long)blockIdx.x * D;
  const int nchunk = D >> 3;
  const int split = D >> 1;
  const int tid = threadIdx.x;
  float x[8];

  bool first = false;
  if (SLOTS) {
    const long long p = pos[blockIdx.x];
    if (p < 0) {  // uniform: before any barrier
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = 0.f;
      for (int c = tid; c < nchunk; c += 256) st8<BF>(y, row + c * 8, x);
      return;
    }
    first = p == 0;
  }

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
      if (SLOTS && first) {
#pragma unroll
        for (int j = 0; j < 8; ++j) pv[j] = 0.f;
      } else {
        ld8<BF>(prev, row + c * 8, pv);
      }
      st8<BF>(y, row + c * 8, pv);
    } else {
      st8<BF>(y, row + c * 8, ln);
    }
    if (prev) st8<BF>(prev, row + c * 8, ln);
  }
}
