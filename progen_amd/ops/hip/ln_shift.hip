// Fused scale-only LayerNorm + token shift, forward and backward.
//
// Implements the LN->shift prologue of both branches
// (reference: progen.py:22,43-46,74-77,132-135) as one memory-bound pass:
// the block normalizes row (b, n) and writes the first ceil(D/2) channels
// into row n+1 (the token shift) and the rest into row n, so the shifted
// activation never exists as a separate tensor.
//
// Memory-bound: vectorized 16 B/lane loads (vec16_t<BF>: 8 bf16 or 4 fp32),
// fp32 statistics, one block per row forward; grid-strided rows backward
// with per-block dweight partials reduced on the host side.
//
// Each kernel has ONE row body, a generic lambda compiled for both values
// of ONE (as dec_ln_shift_kernel is on its ONE flag) and picked once per
// block, inside the kernel, from the row width:
//   ONE   Dv <= LN_BLOCK (every production D): each thread owns <= 1
//         vector, so the row stays in REGISTERS between the passes — no
//         second global read;
//   !ONE  wider rows: a thread owns vectors tid, tid + LN_BLOCK, ... and
//         re-reads them in every pass.
// Every loop over the row ends after one trip when ONE.

#include <type_traits>

#include "common.h"

#define LN_BLOCK 256
#define LN_WAVES (LN_BLOCK / WAVE)

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

// a product rounded on its own. The backward's two sums are taken over
// these, so that the compiler cannot fuse a product into the running sum in
// one instantiation and not in another: left to itself it did, for the wide
// fp32 rows only.
__device__ __forceinline__ float mul_rn(float x, float y) {
#pragma clang fp contract(off)
  return x * y;
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
// The variance is the CENTRED second moment, mean((x - mu)^2), taken in a
// second pass once mu is known (as decode_ln_shift.hip and torch do):
// E[x^2] - mu^2 in fp32 loses (mu/sigma)^2 ulps, 1.5e-5 of rstd at
// mu = 10 sigma. ONE re-reads its registers, !ONE the row, so the cost is
// one more block reduction of the same length.

// RES: fuse the residual add s = x + res (bf16 rounding identical to an
// eager bf16 add); stats and y are computed on s, and s is written out as
// the new residual stream — the separate elementwise add (and its
// backward-side grad accumulation) disappears.
template <bool BF, bool SHIFT, bool RES>
__global__ __launch_bounds__(LN_BLOCK) void ln_shift_fwd_kernel(
    const void* __restrict__ x_, const void* __restrict__ res_,
    const void* __restrict__ g_, void* __restrict__ y_,
    void* __restrict__ s_out_, float* __restrict__ mean,
    float* __restrict__ rstd, int N, int Dv, float eps) {
  // Dv = D / VLEN (vector units); each VEC is 8 bf16 or 4 f32 (16 B)
  using VEC = vec16_t<BF>;
  constexpr int VLEN = vec16<BF>::N;
  const VEC *x = (const VEC*)x_, *res = (const VEC*)res_, *g = (const VEC*)g_;
  VEC *y = (VEC*)y_, *s_out = (VEC*)s_out_;
  const int row = blockIdx.x;
  const int n = row % N;
  const long long base = (long long)row * Dv;
  const int D = Dv * VLEN;
  const int halfv = (D / 2) / VLEN;  // D even, half % VLEN == 0 (host-checked)
  __shared__ float red[LN_WAVES];

  auto body = [&](auto one) {
    constexpr bool ONE = decltype(one)::value;
    VEC v;
    float s = 0.f;
    for (int i = threadIdx.x; i < Dv; i += LN_BLOCK) {
      v = x[base + i];
      if (RES) {
        const VEC rv = res[base + i];
#pragma unroll
        for (int j = 0; j < VLEN; ++j)
          vset<BF>(v, j, vget<BF>(v, j) + vget<BF>(rv, j));
        s_out[base + i] = v;
      }
#pragma unroll
      for (int j = 0; j < VLEN; ++j) s += vget<BF>(v, j);
      if (ONE) break;
    }
    const float mu = ln_block_sum(s, red) / D;

    float ss = 0.f;
    for (int i = threadIdx.x; i < Dv; i += LN_BLOCK) {
      // each thread re-reads the vectors it read (with RES: wrote) above;
      // with RES the summed row was just written: the re-read hits L1/L2
      if (!ONE) v = RES ? s_out[base + i] : x[base + i];
#pragma unroll
      for (int j = 0; j < VLEN; ++j) {
        const float c = vget<BF>(v, j) - mu;
        ss += c * c;
      }
      if (ONE) break;
    }
    const float var = ln_block_sum(ss, red) / D;
    const float rs = rsqrtf(var + eps);
    if (threadIdx.x == 0) {
      mean[row] = mu;
      rstd[row] = rs;
    }

    for (int i = threadIdx.x; i < Dv; i += LN_BLOCK) {
      if (!ONE) v = RES ? s_out[base + i] : x[base + i];
      const VEC gw = g[i];
      VEC o;
#pragma unroll
      for (int j = 0; j < VLEN; ++j)
        vset<BF>(o, j, (vget<BF>(v, j) - mu) * rs * vget<BF>(gw, j));
      if (!SHIFT || i >= halfv) {
        y[base + i] = o;
      } else if (n + 1 < N) {  // shift half -> next row (within the sequence)
        y[base + Dv + i] = o;
      }
      if (ONE) break;
    }
  };
  if (Dv <= LN_BLOCK) body(std::true_type{});
  else body(std::false_type{});

  if (SHIFT && n == 0) {  // first row's shift half is the zero pad
    const VEC z = {};
    for (int i = threadIdx.x; i < halfv; i += LN_BLOCK) y[base + i] = z;
  }
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
// e[d] = upstream grad routed back through the shift:
//   e[d < half] = dy[row+1][d] (0 at the last row of a sequence)
//   e[d >= half] = dy[row][d]
// dx = rs * (e*g - mean(e*g) - xhat * mean(e*g*xhat));  dw += e * xhat

// DS: also add the gradient flowing into the summed stream s (the fused
// variant returns s as a second output; dx then serves as the gradient of
// BOTH addends, since d(x + res) fans out identically).
template <bool BF, bool SHIFT, bool DS>
__global__ __launch_bounds__(LN_BLOCK) void ln_shift_bwd_kernel(
    const void* __restrict__ dy_, const void* __restrict__ ds_,
    const void* __restrict__ x_, const void* __restrict__ g_,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    void* __restrict__ dx_, float* __restrict__ dw_part, int R, int N,
    int Dv) {
  using VEC = vec16_t<BF>;
  constexpr int VLEN = vec16<BF>::N;
  const VEC *dy = (const VEC*)dy_, *ds = (const VEC*)ds_;
  const VEC *x = (const VEC*)x_, *g = (const VEC*)g_;
  VEC* dx = (VEC*)dx_;
  const int D = Dv * VLEN;
  const int halfv = (D / 2) / VLEN;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* dw_lds = (float*)smem;             // D floats
  float* red = (float*)(smem + (size_t)D * 4);  // LN_WAVES floats

  for (int i = threadIdx.x; i < D; i += LN_BLOCK) dw_lds[i] = 0.f;
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
        if (ONE) break;
      }
      __syncthreads();
    }
  };
  if (Dv <= LN_BLOCK) rows(std::true_type{});
  else rows(std::false_type{});

  float* out = dw_part + (size_t)blockIdx.x * D;
  for (int i = threadIdx.x; i < D; i += LN_BLOCK) out[i] = dw_lds[i];
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
// Every instantiation has the same signature, so the three bools index a
// table of the eight: bit 2 is BF, bit 1 SHIFT, bit 0 RES (forward) or DS
// (backward).
#define LN_KERNEL(K, i) K<((i) & 4) != 0, ((i) & 2) != 0, ((i) & 1) != 0>
#define LN_TABLE(K)                                                     \
  {LN_KERNEL(K, 0), LN_KERNEL(K, 1), LN_KERNEL(K, 2), LN_KERNEL(K, 3), \
   LN_KERNEL(K, 4), LN_KERNEL(K, 5), LN_KERNEL(K, 6), LN_KERNEL(K, 7)}

extern "C" {

hipError_t ln_shift_fwd_launch(const void* x, const void* res, const void* g,
                               void* y, void* s_out, float* mean, float* rstd,
                               int R, int N, int D, float eps, bool shift,
                               bool is_bf16, hipStream_t stream) {
  static constexpr decltype(&ln_shift_fwd_kernel<true, true, true>)
      kernels[8] = LN_TABLE(ln_shift_fwd_kernel);
  const int Dv = D / (is_bf16 ? 8 : 4);
  const auto kernel = kernels[is_bf16 * 4 + shift * 2 + (res != nullptr)];
  kernel<<<R, LN_BLOCK, 0, stream>>>(x, res, g, y, s_out, mean, rstd, N, Dv,
                                     eps);
  return hipGetLastError();
}

hipError_t ln_shift_bwd_launch(const void* dy, const void* ds, const void* x,
                               const void* g, const float* mean,
                               const float* rstd, void* dx, float* dw_part,
                               int nblocks, int R, int N, int D, bool shift,
                               bool is_bf16, hipStream_t stream) {
  static constexpr decltype(&ln_shift_bwd_kernel<true, true, true>)
      kernels[8] = LN_TABLE(ln_shift_bwd_kernel);
  const int Dv = D / (is_bf16 ? 8 : 4);
  const size_t lds = (size_t)D * 4 + LN_WAVES * 4 + 16;
  const auto kernel = kernels[is_bf16 * 4 + shift * 2 + (ds != nullptr)];
  kernel<<<nblocks, LN_BLOCK, lds, stream>>>(dy, ds, x, g, mean, rstd, dx,
                                             dw_part, R, N, Dv);
  return hipGetLastError();
}

}  // extern "C"
