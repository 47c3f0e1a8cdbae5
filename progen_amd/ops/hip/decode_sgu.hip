// Decode-step spatial gating row (gMLP SGU) per batch element:
//
//   gl           = LN(gate) * g            h = [xa | gate], each d2 wide
//   hist[b, pos] <- gl
//   out          = xa * (sum_{n <= pos} w[pos, n] * hist[b, n] + bias[pos])
//
// Grid: (d2 / 64 column tiles) x B, 256 threads. The gate row is a few KB,
// so every workgroup recomputes its LN statistics rather than wait for
// another one. A workgroup writes only its own 64 columns of hist[b, pos]
// and takes the n = pos term from registers, so nothing written in this
// launch is read in it. A 64-column slice of a hist row is 8 chunks of 8:
// 8 consecutive lanes hold one row slice and the block's 32 lane groups
// take rows g, g + 32, ... below pos, straight from global memory to
// registers; rows above pos are never read. ``pos`` is read from device
// memory; outside [0, N) the block returns before it touches h, hist or out.

#include "common.h"
#include "decode_kernels.h"

#define TILE 64
#define ROWS_PER_ITER 32
#define UNROLL 4

template <bool BF>
__global__ __launch_bounds__(256) void dec_sgu_kernel(
    const void* __restrict__ h, const void* __restrict__ g, void* hist,
    const void* __restrict__ w, const void* __restrict__ bias,
    const long long* __restrict__ pos_ptr, void* __restrict__ out, int N,
    int d2, float eps) {
  __shared__ float red_a[4], red_b[4];
  __shared__ float part[4][8][8];  // per wave: acc[8], by chunk lane

  const long long pos = *pos_ptr;
  if (pos < 0 || pos >= N) return;  // uniform: before any barrier

  const int b = blockIdx.y;
  const int col0 = blockIdx.x * TILE;
  const int tid = threadIdx.x;
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
        for (int j = 0; j < 8; ++j) acc[j] += wv[u] * hv[u][j];
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
      o[j] = xa[j] * (t + wp * gl[j] + bp);
    }
    st8<BF>(out, (long long)b * d2 + col0 + cl * 8, o);
  }
}

extern "C" hipError_t dec_sgu_launch(const void* h, const void* g, void* hist,
                                     const void* w, const void* bias,
                                     const long long* pos, void* out, int B,
                                     int N, int d2, float eps, bool is_bf16,
                                     hipStream_t stream) {
  const dim3 grid(d2 / TILE, B);
  if (is_bf16)
    dec_sgu_kernel<true><<<grid, 256, 0, stream>>>(h, g, hist, w, bias, pos,
                                                   out, N, d2, eps);
  else
    dec_sgu_kernel<false><<<grid, 256, 0, stream>>>(h, g, hist, w, bias, pos,
                                                    out, N, d2, eps);
  return hipGetLastError();
}
