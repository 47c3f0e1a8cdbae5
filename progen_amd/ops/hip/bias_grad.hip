// Bias gradients summed where the gradient is produced.
//
// The output gradient of a biased linear is summed over its rows for the
// bias gradient. For proj_in (GLU layers) that gradient is the dh glu_bwd
// stores; for to_out and ff.proj_out it is the dx the next ln_shift_res
// backward stores. The kernels here are those two backward kernels (their
// bodies are the shared glu_bwd_body.h and ln_shift_bwd_body.h) plus a
// per-column fp32 sum of THE VALUES THEY STORE, i.e. of the rounded bf16 a
// separate column reduce would have read, written as one partial row per
// block (stripe). The partials are summed in a fixed order by the caller
// (bindings.cpp); there is no atomic anywhere on this path, so two calls on
// the same inputs give the same bits.

#include "glu_bwd_body.h"
#include "ln_shift_bwd_body.h"

// A thread owns its columns (one vector in each half of h) for the whole
// stripe loop: 2 * VLEN private accumulators, no cross-thread reduction.
// part: [gridDim.y, 2H] fp32.
template <bool BF>
__global__ __launch_bounds__(GLU_BLOCK) void glu_bwd_db_kernel(
    const void* __restrict__ dy_, const void* __restrict__ h_,
    void* __restrict__ dh_, float* __restrict__ part, long long rows,
    int Hv) {
  using VEC = vec16_t<BF>;
  constexpr int VLEN = vec16<BF>::N;
  const VEC *dy = (const VEC*)dy_, *h = (const VEC*)h_;
  VEC* dh = (VEC*)dh_;
  const int i = blockIdx.x * GLU_BLOCK + (int)threadIdx.x;
  if (i >= Hv) return;
  float sa[VLEN], sg[VLEN];
#pragma unroll
  for (int j = 0; j < VLEN; ++j) sa[j] = sg[j] = 0.f;
  for (long long row = blockIdx.y; row < rows; row += gridDim.y) {
    VEC da, dg;
    glu_bwd_row<BF>(dy, h, dh, row, Hv, i, da, dg);
    // the values as stored, read back out of the vectors
    opaque_vec(da);
    opaque_vec(dg);
#pragma unroll
    for (int j = 0; j < VLEN; ++j) {
      sa[j] += vget<BF>(da, j);
      sg[j] += vget<BF>(dg, j);
    }
  }
  // 16 B stores: a vector of VLEN floats is VLEN/4 of them
  f32x4* out = (f32x4*)(part + (size_t)blockIdx.y * 2 * Hv * VLEN);
#pragma unroll
  for (int q = 0; q < VLEN / 4; ++q) {
    out[i * (VLEN / 4) + q] =
        f32x4{sa[4 * q], sa[4 * q + 1], sa[4 * q + 2], sa[4 * q + 3]};
    out[(Hv + i) * (VLEN / 4) + q] =
        f32x4{sg[4 * q], sg[4 * q + 1], sg[4 * q + 2], sg[4 * q + 3]};
  }
}

template <bool BF, bool SHIFT, bool DS>
__global__ __launch_bounds__(LN_BLOCK) void ln_shift_bwd_db_kernel(
    const void* __restrict__ dy_, const void* __restrict__ ds_,
    const void* __restrict__ x_, const void* __restrict__ g_,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    void* __restrict__ dx_, float* __restrict__ dw_part,
    float* __restrict__ db_part, int R, int N, int Dv) {
  ln_shift_bwd_body<BF, SHIFT, DS, true>(dy_, ds_, x_, g_, mean, rstd, dx_,
                                         dw_part, db_part, R, N, Dv);
}

extern "C" {

// Row stripes (grid y, and rows of ``part``) of glu_bwd_db at this shape.
// glu_bwd spreads about 4096 blocks; here every stripe costs a partial row
// that is written and read back, so the grid is about 1024 blocks: 4 per CU
// on 256 CUs, all resident at once at any occupancy from 4 waves per SIMD up,
// with each block's rows equal to within one.
int glu_bwd_db_stripes(long long rows, int H, bool is_bf16) {
  const int Hv = H / (is_bf16 ? 8 : 4);
  const int gx = (Hv + GLU_BLOCK - 1) / GLU_BLOCK;
  long long gy = 1024 / gx;
  if (gy < 1) gy = 1;
  if (gy > rows) gy = rows;
  return (int)gy;
}

hipError_t glu_bwd_db_launch(const void* dy, const void* h, void* dh,
                             float* part, int stripes, long long rows, int H,
                             bool is_bf16, hipStream_t stream) {
  const int Hv = H / (is_bf16 ? 8 : 4);
  const dim3 grid((Hv + GLU_BLOCK - 1) / GLU_BLOCK, (unsigned)stripes);
  if (is_bf16)
    glu_bwd_db_kernel<true><<<grid, GLU_BLOCK, 0, stream>>>(dy, h, dh, part,
                                                            rows, Hv);
  else
    glu_bwd_db_kernel<false><<<grid, GLU_BLOCK, 0, stream>>>(dy, h, dh, part,
                                                             rows, Hv);
  return hipGetLastError();
}

hipError_t ln_shift_bwd_db_launch(const void* dy, const void* ds,
                                  const void* x, const void* g,
                                  const float* mean, const float* rstd,
                                  void* dx, float* dw_part, float* db_part,
                                  int nblocks, int R, int N, int D, bool shift,
                                  bool is_bf16, hipStream_t stream) {
  static constexpr decltype(&ln_shift_bwd_db_kernel<true, true, true>)
      kernels[8] = LN_TABLE(ln_shift_bwd_db_kernel);
  const int Dv = D / (is_bf16 ? 8 : 4);
  const size_t lds = (size_t)D * 8 + LN_WAVES * 4 + 16;  // dw, db, red
  const auto kernel = kernels[is_bf16 * 4 + shift * 2 + (ds != nullptr)];
  kernel<<<nblocks, LN_BLOCK, lds, stream>>>(dy, ds, x, g, mean, rstd, dx,
                                             dw_part, db_part, R, N, Dv);
  return hipGetLastError();
}

}  // extern "C"
