// Body of the decode-step spatial gating row (decode_sgu.hip), written once
// for the scalar kernel and for the slot kernel (decode_slots.hip).
//
// SLOTS = false: every row runs at the one position *pos_ptr; outside [0, N)
//                the block returns before it touches anything.
// SLOTS = true:  batch row b runs at pos_ptr[b]. Outside [0, N) the row is
//                idle: its tile of out is written as zeros and h and hist are
//                not touched. Only history rows [0, pos) are read, which a
//                request that started at 0 wrote itself.
//
// The scalar and the slot kernel must give the same bits, so no fused
// multiply-add is left to the compiler: it contracts a product and a sum only
// where both land in one basic block, and which ones do differs between the
// two instantiations. Contraction is off in this body and every fma is
// written out.
#pragma once

#include "common.h"

#define DEC_SGU_TILE 64
#define DEC_SGU_ROWS_PER_ITER 32
#define DEC_SGU_UNROLL 4

template <bool BF, bool SLOTS>
__device__ __forceinline__ void dec_sgu_body(
    const void* __restrict__ h, const void* __restrict__ g, void* hist,
    const void* __restrict__ w, const void* __restrict__ bias,
    const long long* __restrict__ pos_ptr, void* __restrict__ out, int N,
    int d2, float eps) {
#pragma clang fp contract(off)
  constexpr int TILE = DEC_SGU_TILE;
  constexpr int ROWS_PER_ITER = DEC_SGU_ROWS_PER_ITER;
  constexpr int UNROLL = DEC_SGU_UNROLL;
  __shared__ float red_a[4], red_b[4];
  __shared__ float part[4][8][8];  // per wave: acc[8], by chunk lane

  const int b = blockIdx.y;
  const int col0 = blockIdx.x * TILE;
  const int tid = threadIdx.x;
  const long long pos = SLOTS ? pos_ptr[b] : *pos_ptr;
  if (pos < 0 || pos >= N) {  // uniform: before any barrier
    if (SLOTS && tid < 8) {
      float z[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) z[j] = 0.f;
      st8<BF>(out, (long long)b * d2 + col0 + tid * 8, z);
    }
    return;
  }

  const int wave = tid >> 6, lane = tid & 63;
  const int cl = lane & 7;
  const int grp = wave * 8 + (lane >> 3);
  const long long xa_row = (long long)b * 2 * d2;
  const long long gate_row = xa_row + d2;

  // ---- LN statistics of the whole gate row (two passes, L1-resident) -----
  const int nchunk = d2 >> 3;
  float s = 0.f;
  for (int c = tid; c < nchunk; c += 256) {
    float x[8];
    ld8<BF>(h, gate_row + c * 8, x);
#pragma unroll
    for (int j = 0; j < 8; ++j) s += x[j];
  }
  const float mu = block256_sum(s, red_a) / d2;
  float ss = 0.f;
  for (int c = tid; c < nchunk; c += 256) {
    float x[8];
    ld8<BF>(h, gate_row + c * 8, x);
#pragma unroll
    for (int j = 0; j < 8; ++j) ss += (x[j] - mu) * (x[j] - mu);
  }
  const float rs = rsqrtf(block256_sum(ss, red_b) / d2 + eps);

  // ---- rows below pos ------------------------------------------------------
  const long long hbase = (long long)b * N * d2 + col0 + cl * 8;
  const long long wrow = pos * N;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  const int nrows = (int)pos;
  for (int r0 = grp; r0 < nrows; r0 += ROWS_PER_ITER * UNROLL) {
    float hv[UNROLL][8], wv[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int r = r0 + u * ROWS_PER_ITER;
      if (r < nrows) {
        ld8<BF>(hist, hbase + (long long)r * d2, hv[u]);
        wv[u] = ld1<BF>(w, wrow + r);
      }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int r = r0 + u * ROWS_PER_ITER;
      if (r < nrows) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = fmaf(wv[u], hv[u][j], acc[j]);
      }
    }
  }
#pragma unroll
  for (int off = 8; off < 64; off <<= 1) {
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += __shfl_xor(acc[j], off, 64);
  }
  if (lane < 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) part[wave][j][cl] = acc[j];
  }
  __syncthreads();

  // ---- this tile's slice of the new row, the n = pos term, the gate -------
  if (tid < 8) {
    float x[8], gv[8], gl[8], xa[8], o[8];
    ld8<BF>(h, gate_row + col0 + cl * 8, x);
    ld8<BF>(g, col0 + cl * 8, gv);
    ld8<BF>(h, xa_row + col0 + cl * 8, xa);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      gl[j] = round_trip<BF>((x[j] - mu) * rs * gv[j]);
    st8<BF>(hist, hbase + pos * d2, gl);
    const float wp = ld1<BF>(w, wrow + pos);
    const float bp = ld1<BF>(bias, pos);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float t = part[0][j][cl] + part[1][j][cl] + part[2][j][cl] +
                      part[3][j][cl];
      o[j] = xa[j] * (fmaf(wp, gl[j], t) + bp);
    }
    st8<BF>(out, (long long)b * d2 + col0 + cl * 8, o);
  }
}
