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

#include <type_traits>  // the forward's body is picked by std::true_type too

#include "ln_common.h"
#include "ln_shift_bwd_body.h"

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
// The body is ln_shift_bwd_body.h, shared with the variant that also sums
// dx per column (bias_grad.hip).
template <bool BF, bool SHIFT, bool DS>
__global__ __launch_bounds__(LN_BLOCK) void ln_shift_bwd_kernel(
    const void* __restrict__ dy_, const void* __restrict__ ds_,
    const void* __restrict__ x_, const void* __restrict__ g_,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    void* __restrict__ dx_, float* __restrict__ dw_part, int R, int N,
    int Dv) {
  ln_shift_bwd_body<BF, SHIFT, DS, false>(dy_, ds_, x_, g_, mean, rstd, dx_,
                                          dw_part, nullptr, R, N, Dv);
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
// Every instantiation has the same signature, so the three bools index a
// table of the eight: bit 2 is BF, bit 1 SHIFT, bit 0 RES (forward) or DS
// (backward): LN_TABLE of ln_common.h.

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
