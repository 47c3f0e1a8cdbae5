// Body of the decode-step attention row (decode_attn.hip), written once for
// the scalar kernel and for the slot kernel (decode_slots.hip).
//
// SLOTS = false: every (b, h) runs at the one position *pos_ptr; outside
//                [0, N) the block returns before it touches anything.
// SLOTS = true:  batch row b runs at pos_ptr[b]. Outside [0, N) the row is
//                idle: its out row is written as zeros and qkv and the caches
//                are not touched. A slot's band holds only rows its own
//                request wrote: the band starts at max(0, w0 - window) and the
//                zero lookback window below row 0 is synthesised, never loaded.
//
// Unlike decode_ln_shift_body.h and decode_sgu_body.h this body leaves
// contraction to the compiler and pins a single fma (the last combine). With
// contraction off and every fma written out, the two instantiations agree by
// construction, but the scalar kernel no longer computes what it always has:
// as compiled, it fuses six of the eight acc[j] * a + e * vv[u][j] of a cached
// row and leaves two as a product and a sum, which no plain source spells
// out. So the arithmetic of the scalar kernel is kept, the one sum that the
// compiler contracted differently in the two kernels is explicit, and
// tests/test_gpu_decode_slots.py holds the two to the same bits in fp32.
#pragma once

#include <math.h>

#include "common.h"

#define DEC_ATTN_DH 64
#define DEC_ATTN_ROWS_PER_ITER 32  // lane groups per block
#define DEC_ATTN_UNROLL 4  // independent K/V row loads in flight per group

// interleaved rotary on an 8-element chunk (4 pairs), result as stored
template <bool BF>
__device__ __forceinline__ void rope8(float* x, const float* sv,
                                      const float* cv) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const float x0 = x[2 * p], x1 = x[2 * p + 1];
    const float s = sv[2 * p], c = cv[2 * p];
    x[2 * p] = round_trip<BF>(x0 * c - x1 * s);
    x[2 * p + 1] = round_trip<BF>(x1 * c + x0 * s);
  }
}

template <bool BF, bool SLOTS>
__device__ __forceinline__ void dec_attn_body(
    const void* __restrict__ qkv, const float* __restrict__ rsin,
    const float* __restrict__ rcos, const long long* __restrict__ pos_ptr,
    void* k_cache, void* v_cache, void* __restrict__ out, int H, int N,
    int window) {
  constexpr int DH = DEC_ATTN_DH;
  constexpr int ROWS_PER_ITER = DEC_ATTN_ROWS_PER_ITER;
  constexpr int UNROLL = DEC_ATTN_UNROLL;
  __shared__ float part[4][10][8];  // per wave: m, l, acc[8], by chunk lane

  const int b = blockIdx.x / H, hd = blockIdx.x % H;
  const int tid = threadIdx.x;
  const long long HD = (long long)H * DH;
  const long long pos = SLOTS ? pos_ptr[b] : *pos_ptr;
  if (pos < 0 || pos >= N) {  // uniform: before any barrier
    if (SLOTS && tid < 8) {
      float z[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) z[j] = 0.f;
      st8<BF>(out, (long long)b * HD + (long long)hd * DH + tid * 8, z);
    }
    return;
  }

  const int wave = tid >> 6, lane = tid & 63;
  const int cl = lane & 7;             // chunk within the 64-wide row
  const int grp = wave * 8 + (lane >> 3);
  const int d0 = cl * 8;

  // ---- q, k, v of this head: rotate at row pos --------------------------
  float sv[8], cv[8], q[8], kc[8], vc[8];
  *(f32x4*)(sv) = *(const f32x4*)(rsin + pos * DH + d0);
  *(f32x4*)(sv + 4) = *(const f32x4*)(rsin + pos * DH + d0 + 4);
  *(f32x4*)(cv) = *(const f32x4*)(rcos + pos * DH + d0);
  *(f32x4*)(cv + 4) = *(const f32x4*)(rcos + pos * DH + d0 + 4);
  const long long qoff = (long long)b * 3 * HD + (long long)hd * DH + d0;
  ld8<BF>(qkv, qoff, q);
  ld8<BF>(qkv, qoff + HD, kc);
  ld8<BF>(qkv, qoff + 2 * HD, vc);
  rope8<BF>(q, sv, cv);
  rope8<BF>(kc, sv, cv);
  rope8<BF>(vc, sv, cv);

  const long long base = ((long long)b * H + hd) * N * DH + d0;
  const float scale = 0.125f;  // 64^-0.5

  // ---- running state; group 0 starts from the current row ---------------
  float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  if (grp == 0) {
    st8<BF>(k_cache, base + pos * DH, kc);
    st8<BF>(v_cache, base + pos * DH, vc);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += q[j] * kc[j];
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    s *= scale;
    if (pos < window) {
      // zero lookback window: ``window`` logits of 0, values 0
      m = fmaxf(s, 0.f);
      const float e = expf(s - m);
      l = e + (float)window * expf(-m);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = e * vc[j];
    } else {
      m = s;
      l = 1.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = vc[j];
    }
  }

  // ---- cached rows [start, pos) -------------------------------------------
  const int w0 = (int)(pos / window) * window;
  const int start = w0 >= window ? w0 - window : 0;
  const int nrows = (int)pos - start;
  for (int r0 = grp; r0 < nrows; r0 += ROWS_PER_ITER * UNROLL) {
    float kk[UNROLL][8], vv[UNROLL][8];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int r = r0 + u * ROWS_PER_ITER;
      if (r < nrows) {
        const long long off = base + (long long)(start + r) * DH;
        ld8<BF>(k_cache, off, kk[u]);
        ld8<BF>(v_cache, off, vv[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int r = r0 + u * ROWS_PER_ITER;
      if (r < nrows) {  // uniform over the 8 lanes of a group
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) s += q[j] * kk[u][j];
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        s += __shfl_xor(s, 4, 64);
        s *= scale;
        const float mn = fmaxf(m, s);
        const float a = expf(m - mn);  // 0 on the first row (m = -inf)
        const float e = expf(s - mn);
        l = l * a + e;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = acc[j] * a + e * vv[u][j];
        m = mn;
      }
    }
  }

  // ---- combine the 8 groups of a wave, then the 4 waves -------------------
  float mw = m;
  mw = fmaxf(mw, __shfl_xor(mw, 8, 64));
  mw = fmaxf(mw, __shfl_xor(mw, 16, 64));
  mw = fmaxf(mw, __shfl_xor(mw, 32, 64));
  // a group (or a whole wave) without rows has m = -inf and weight 0
  const float wgt = (m == -INFINITY) ? 0.f : expf(m - mw);
  l *= wgt;
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] *= wgt;
#pragma unroll
  for (int off = 8; off < 64; off <<= 1) {
    l += __shfl_xor(l, off, 64);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += __shfl_xor(acc[j], off, 64);
  }
  if (lane < 8) {
    part[wave][0][cl] = mw;
    part[wave][1][cl] = l;
#pragma unroll
    for (int j = 0; j < 8; ++j) part[wave][2 + j][cl] = acc[j];
  }
  __syncthreads();
  if (tid < 8) {
    float mb = part[0][0][cl];  // wave 0 holds the current row: finite
#pragma unroll
    for (int w = 1; w < 4; ++w) mb = fmaxf(mb, part[w][0][cl]);
    float lb = 0.f, o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float mv = part[w][0][cl];
      const float f = (mv == -INFINITY) ? 0.f : expf(mv - mb);
      lb += f * part[w][1][cl];
      // written out as an fma: left to the compiler, this sum is contracted
      // in the scalar kernel and not in the slot kernel (a product and a sum
      // are fused only where both land in one basic block)
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = fmaf(f, part[w][2 + j][cl], o[j]);
    }
    const float inv = 1.f / lb;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] *= inv;
    st8<BF>(out, (long long)b * HD + (long long)hd * DH + d0, o);
  }
}
