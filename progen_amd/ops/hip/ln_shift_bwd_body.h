// Body of the fused LN + token-shift backward, written once for
// ln_shift_bwd_kernel (ln_shift.hip) and ln_shift_bwd_db_kernel
// (bias_grad.hip).
//
// e[d] = upstream grad routed back through the shift:
//   e[d < half] = dy[row+1][d] (0 at the last row of a sequence)
//   e[d >= half] = dy[row][d]
// dx = rs * (e*g - mean(e*g) - xhat * mean(e*g*xhat));  dw += e * xhat
//
// DS: also add the gradient flowing into the summed stream s (the fused
// variant returns s as a second output; dx then serves as the gradient of
// BOTH addends, since d(x + res) fans out identically).
//
// DB: also sum the STORED dx (rounded to the storage type, the ds addend
// included) per column into a second LDS accumulator next to dw's, flushed
// the same way to ``db_part``: dx is the output gradient of the linear that
// produced the res addend, so its column sum is that linear's bias gradient.
#pragma once

#include <type_traits>

#include "ln_common.h"

// a product rounded on its own. The backward's two sums are taken over
// these, so that the compiler cannot fuse a product into the running sum in
// one instantiation and not in another: left to itself it did, for the wide
// fp32 rows only.
__device__ __forceinline__ float mul_rn(float x, float y) {
#pragma clang fp contract(off)
  return x * y;
}

// Dynamic LDS: D floats per column accumulator (one, or two with DB), then
// LN_WAVES floats of block-sum scratch.
template <bool BF, bool SHIFT, bool DS, bool DB>
__device__ __forceinline__ void ln_shift_bwd_body(
    const void* __restrict__ dy_, const void* __restrict__ ds_,
    const void* __restrict__ x_, const void* __restrict__ g_,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    void* __restrict__ dx_, float* __restrict__ dw_part,
    float* __restrict__ db_part, int R, int N, int Dv) {
  using VEC = vec16_t<BF>;
  constexpr int VLEN = vec16<BF>::N;
  const VEC *dy = (const VEC*)dy_, *ds = (const VEC*)ds_;
  const VEC *x = (const VEC*)x_, *g = (const VEC*)g_;
  VEC* dx = (VEC*)dx_;
  const int D = Dv * VLEN;
  const int halfv = (D / 2) / VLEN;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* dw_lds = (float*)smem;             // D floats
  float* db_lds = dw_lds + D;               // D floats, only with DB
  float* red = (float*)(smem + (size_t)D * 4 * (DB ? 2 : 1));  // LN_WAVES floats

  for (int i = threadIdx.x; i < D; i += LN_BLOCK) {
    dw_lds[i] = 0.f;
    if (DB) db_lds[i] = 0.f;
  }
  __syncthreads();

  // the block's rows. The width is tested once, outside the row loop: with
  // both bodies inside one loop the compiler has to assume, at the top of a
  // row, that loads of the other body are still in flight, and its wait for
  // them also drains the dx stores of the row before.
  auto rows = [&](auto one) {
    constexpr bool ONE = decltype(one)::value;
    for (int row = blockIdx.x; row < R; row += gridDim.x) {
      const int n = row % N;
      const long long base = (long long)row * Dv;
      const float mu = mean[row];
      const float rs = rstd[row];
      const float inv_d = 1.0f / D;

      // vector i of the row's operands; when ONE they are fetched once and
      // stay in registers between the two passes
      VEC e, v, gw, dsv;
      // ds goes first although it is used last: loads complete in order,
      // so the first pass's wait for gw then leaves none in flight. With ds
      // last, the compiler guards the next row's first loads against it
      // (a wave without a vector skips the second pass, where it is waited
      // for), and that wait also drains the dx stores of this row.
      auto fetch = [&](int i) {
        if (DS) dsv = ds[base + i];
        if (!SHIFT || i >= halfv) e = dy[base + i];
        else if (n + 1 < N) e = dy[base + Dv + i];
        else e = VEC{};
        v = x[base + i];
        gw = g[i];
      };

      float a = 0.f, bsum = 0.f;  // a = sum(e*g*xhat), bsum = sum(e*g)
      for (int i = threadIdx.x; i < Dv; i += LN_BLOCK) {
        fetch(i);
#pragma unroll
        for (int j = 0; j < VLEN; ++j) {
          const float ej = vget<BF>(e, j), gj = vget<BF>(gw, j);
          const float xh = (vget<BF>(v, j) - mu) * rs;
          const float eg = mul_rn(ej, gj);
          a += mul_rn(eg, xh);
          bsum += eg;
        }
        if (ONE) break;
      }
      a = ln_block_sum(a, red);
      bsum = ln_block_sum(bsum, red);

      for (int i = threadIdx.x; i < Dv; i += LN_BLOCK) {
        if (!ONE) fetch(i);
        VEC o;
#pragma unroll
        for (int j = 0; j < VLEN; ++j) {
          const float ej = vget<BF>(e, j), gj = vget<BF>(gw, j);
          const float xh = (vget<BF>(v, j) - mu) * rs;
          float dxv = rs * (ej * gj - bsum * inv_d - xh * a * inv_d);
          if (DS) dxv += vget<BF>(dsv, j);
          vset<BF>(o, j, dxv);
          dw_lds[i * VLEN + j] += ej * xh;  // thread-private index: no race
        }
        dx[base + i] = o;
        if (DB) {  // the values as stored, read back out of the vector
          opaque_vec(o);
#pragma unroll
          for (int j = 0; j < VLEN; ++j)
            db_lds[i * VLEN + j] += vget<BF>(o, j);
        }
        if (ONE) break;
      }
      __syncthreads();
    }
  };
  if (Dv <= LN_BLOCK) rows(std::true_type{});
  else rows(std::false_type{});

  float* out = dw_part + (size_t)blockIdx.x * D;
  for (int i = threadIdx.x; i < D; i += LN_BLOCK) out[i] = dw_lds[i];
  if (DB) {
    float* bout = db_part + (size_t)blockIdx.x * D;
    for (int i = threadIdx.x; i < D; i += LN_BLOCK) bout[i] = db_lds[i];
  }
}
