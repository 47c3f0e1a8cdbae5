// GLU-GELU epilogue of the feedforward (reference: progen.py:139-143):
//   glu:  y = a * gelu(g)  with (a, g) = split(h, 2, dim=-1)
//   gelu: y = gelu(h)
// Memory-bound elementwise kernels, one 16 B vector (vec16_t<BF>) per lane
// and trip, grid-stride.

#include "common.h"
#include "glu_bwd_body.h"  // GLU_BLOCK, glu_bwd_row

// 2-D grid (columns x row-stripes): the flat-index form cost two
// 64-bit integer divisions per iteration — a long VALU sequence on a
// kernel this loop-dense
template <bool BF>
__global__ __launch_bounds__(GLU_BLOCK) void glu_fwd_kernel(
    const void* __restrict__ h_, void* __restrict__ y_, long long rows,
    int Hv) {
  using VEC = vec16_t<BF>;
  const VEC* h = (const VEC*)h_;
  VEC* y = (VEC*)y_;
  const int i = blockIdx.x * GLU_BLOCK + (int)threadIdx.x;
  if (i >= Hv) return;
  for (long long row = blockIdx.y; row < rows; row += gridDim.y) {
    const VEC va = h[row * 2 * Hv + i];
    const VEC vg = h[row * 2 * Hv + Hv + i];
    VEC o;
#pragma unroll
    for (int j = 0; j < vec16<BF>::N; ++j)
      vset<BF>(o, j, vget<BF>(va, j) * gelu_tanh(vget<BF>(vg, j)));
    y[row * Hv + i] = o;
  }
}

template <bool BF>
__global__ __launch_bounds__(GLU_BLOCK) void glu_bwd_kernel(
    const void* __restrict__ dy_, const void* __restrict__ h_,
    void* __restrict__ dh_, long long rows, int Hv) {
  using VEC = vec16_t<BF>;
  const VEC *dy = (const VEC*)dy_, *h = (const VEC*)h_;
  VEC* dh = (VEC*)dh_;
  const int i = blockIdx.x * GLU_BLOCK + (int)threadIdx.x;
  if (i >= Hv) return;
  for (long long row = blockIdx.y; row < rows; row += gridDim.y) {
    VEC da, dg;
    glu_bwd_row<BF>(dy, h, dh, row, Hv, i, da, dg);
  }
}

template <bool BF>
__global__ __launch_bounds__(GLU_BLOCK) void gelu_fwd_kernel(
    const void* __restrict__ h_, void* __restrict__ y_, long long total) {
  using VEC = vec16_t<BF>;
  const VEC* h = (const VEC*)h_;
  VEC* y = (VEC*)y_;
  for (long long idx = blockIdx.x * (long long)GLU_BLOCK + threadIdx.x;
       idx < total; idx += (long long)gridDim.x * GLU_BLOCK) {
    const VEC v = h[idx];
    VEC o;
#pragma unroll
    for (int j = 0; j < vec16<BF>::N; ++j)
      vset<BF>(o, j, gelu_tanh(vget<BF>(v, j)));
    y[idx] = o;
  }
}

template <bool BF>
__global__ __launch_bounds__(GLU_BLOCK) void gelu_bwd_kernel(
    const void* __restrict__ dy_, const void* __restrict__ h_,
    void* __restrict__ dh_, long long total) {
  using VEC = vec16_t<BF>;
  const VEC *dy = (const VEC*)dy_, *h = (const VEC*)h_;
  VEC* dh = (VEC*)dh_;
  for (long long idx = blockIdx.x * (long long)GLU_BLOCK + threadIdx.x;
       idx < total; idx += (long long)gridDim.x * GLU_BLOCK) {
    const VEC v = h[idx];
    const VEC vdy = dy[idx];
    VEC o;
#pragma unroll
    for (int j = 0; j < vec16<BF>::N; ++j)
      vset<BF>(o, j, vget<BF>(vdy, j) * gelu_tanh_grad(vget<BF>(v, j)));
    dh[idx] = o;
  }
}

static inline int glu_grid(long long total) {
  long long g = (total + GLU_BLOCK - 1) / GLU_BLOCK;
  if (g > 2048) g = 2048;  // grid-stride the rest (G11)
  return (int)g;
}

// 2-D grid for the split (glu) kernels: x covers the Hv columns, y
// row-stripes sized so x*y lands near 4096 blocks
static inline dim3 glu_grid2(long long rows, int Hv) {
  int gx = (Hv + GLU_BLOCK - 1) / GLU_BLOCK;
  long long gy = 4096 / gx;
  if (gy < 1) gy = 1;
  if (gy > rows) gy = rows;
  return dim3(gx, (unsigned)gy);
}

extern "C" {

hipError_t glu_fwd_launch(const void* h, void* y, long long rows, int H,
                          bool is_bf16, hipStream_t stream) {
  const int Hv = H / (is_bf16 ? 8 : 4);
  const dim3 grid = glu_grid2(rows, Hv);
  if (is_bf16)
    glu_fwd_kernel<true><<<grid, GLU_BLOCK, 0, stream>>>(h, y, rows, Hv);
  else
    glu_fwd_kernel<false><<<grid, GLU_BLOCK, 0, stream>>>(h, y, rows, Hv);
  return hipGetLastError();
}

hipError_t glu_bwd_launch(const void* dy, const void* h, void* dh,
                          long long rows, int H, bool is_bf16,
                          hipStream_t stream) {
  const int Hv = H / (is_bf16 ? 8 : 4);
  const dim3 grid = glu_grid2(rows, Hv);
  if (is_bf16)
    glu_bwd_kernel<true><<<grid, GLU_BLOCK, 0, stream>>>(dy, h, dh, rows, Hv);
  else
    glu_bwd_kernel<false><<<grid, GLU_BLOCK, 0, stream>>>(dy, h, dh, rows, Hv);
  return hipGetLastError();
}

hipError_t gelu_fwd_launch(const void* h, void* y, long long total_elems,
                           bool is_bf16, hipStream_t stream) {
  const long long tv = total_elems / (is_bf16 ? 8 : 4);
  if (is_bf16)
    gelu_fwd_kernel<true><<<glu_grid(tv), GLU_BLOCK, 0, stream>>>(h, y, tv);
  else
    gelu_fwd_kernel<false><<<glu_grid(tv), GLU_BLOCK, 0, stream>>>(h, y, tv);
  return hipGetLastError();
}

hipError_t gelu_bwd_launch(const void* dy, const void* h, void* dh,
                           long long total_elems, bool is_bf16,
                           hipStream_t stream) {
  const long long tv = total_elems / (is_bf16 ? 8 : 4);
  if (is_bf16)
    gelu_bwd_kernel<true><<<glu_grid(tv), GLU_BLOCK, 0, stream>>>(dy, h, dh, tv);
  else
    gelu_bwd_kernel<false><<<glu_grid(tv), GLU_BLOCK, 0, stream>>>(dy, h, dh, tv);
  return hipGetLastError();
}

}  // extern "C"
