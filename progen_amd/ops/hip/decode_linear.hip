// Decode-step linear with a fused epilogue, for 1..32 rows:
//
//   out[B, N'] = act(x[B, K] @ W[N, K]^T + bias[N])
//
//   act none / tanh-GELU   N' = N
//   act GLU                N' = N/2, out[:, j] = (a_j + bias_j) *
//                          gelu(g_{j+N/2} + bias_{j+N/2})
//
// W is nn.Linear's [N][K] with K contiguous, so a weight row is a stream.
// A workgroup owns 16 output columns (GLU: the 16 value rows AND the 16
// gate rows they pair with) and nw = blockDim.x / 64 waves split K between
// them: wave w takes the 64-element K-steps w, w + nw, ... In a step lane l
// reads 16 consecutive elements of weight row (l & 15) at K offset
// 16 * (l >> 4) — for bf16 two 16 B loads, and the four lanes of a row read
// one whole 128 B line — straight from global memory into registers, a few
// steps ahead of their use. Nothing is staged through LDS; x is a few KB
// and comes from L1/L2.
//
// Two arithmetic paths:
//   vec    fp32 FMAs, 4 batch rows per workgroup (grid.y = ceil(B / 4)):
//          fp32 always, bf16 for B <= DEC_LINEAR_VEC_MAX_B;
//   mfma   bf16 only, mfma_f32_16x16x32_bf16 with the weight rows as the A
//          fragment and the batch as the 16 columns of B. A lane's 16
//          elements are two consecutive MFMA K-steps (a dot product does
//          not care about K order as long as x is read in the same order).
//          Batch columns >= B are fed zeros and never loaded; B > 16 takes
//          a second batch tile against the same A fragments.
//
// The waves' partial sums meet in LDS and are added in wave order by the
// threads that then add the bias, apply the activation on the fp32 sum and
// store, rounding once. No atomics, no split-K across workgroups, nothing
// written in this launch is read in it: the kernel is as capturable and as
// bit-reproducible as the other decode kernels.

#include "common.h"
#include "decode_linear_kernels.h"

#define TN 16    // output columns per workgroup
#define KSTEP 64 // K elements per wave step
#define VEC_BT 4 // batch rows per workgroup on the vec path

enum { ACT_NONE = 0, ACT_GELU = 1, ACT_GLU = 2 };

template <bool BF>
__device__ __forceinline__ void ld16(const void* p, long long idx, float* x) {
  ld8<BF>(p, idx, x);
  ld8<BF>(p, idx + 8, x + 8);
}

// 16 consecutive elements as loaded: in-flight weights wait in the storage
// type (8 VGPRs for bf16) and are widened only where they are used
template <bool BF>
struct raw16 {
  f32x4 v[4];
};
template <>
struct raw16<true> {
  bf16x8 v[2];
};

template <bool BF>
__device__ __forceinline__ raw16<BF> ldraw16(const void* p, long long idx) {
  raw16<BF> r;
  if constexpr (BF) {
    r.v[0] = *(const bf16x8*)((const short*)p + idx);
    r.v[1] = *(const bf16x8*)((const short*)p + idx + 8);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      r.v[q] = *(const f32x4*)((const float*)p + idx + 4 * q);
  }
  return r;
}

template <bool BF>
__device__ __forceinline__ void widen16(const raw16<BF>& r, float* x) {
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if constexpr (BF) x[j] = bf2f(r.v[j >> 3][j & 7]);
    else x[j] = r.v[j >> 2][j & 3];
  }
}

// sum over the waves in wave order, bias, activation, one rounding.
// ``part`` is [wave][half][tile-local index]; ``idx`` the tile-local index
// of output (b, n0 + nl), ``stride`` the floats of one wave.
template <bool BF, int ACT>
__device__ __forceinline__ void epilogue(const float* part, int nw,
                                         int stride, int hstride, int idx,
                                         const void* bias, void* out, int b,
                                         int n0, int nl, int N) {
  float a = 0.f, g = 0.f;
  for (int w = 0; w < nw; ++w) {
    a += part[w * stride + idx];
    if constexpr (ACT == ACT_GLU) g += part[w * stride + hstride + idx];
  }
  const int half = N >> 1;
  if (bias) {
    a += ld1<BF>(bias, n0 + nl);
    if constexpr (ACT == ACT_GLU) g += ld1<BF>(bias, half + n0 + nl);
  }
  if constexpr (ACT == ACT_GLU) {
    st1<BF>(out, (long long)b * half + n0 + nl, a * gelu_tanh(g));
  } else if constexpr (ACT == ACT_GELU) {
    st1<BF>(out, (long long)b * N + n0 + nl, gelu_tanh(a));
  } else {
    st1<BF>(out, (long long)b * N + n0 + nl, a);
  }
}

// ---------------------------------------------------------------------------
// vec path
// ---------------------------------------------------------------------------

template <bool BF, int ACT>
__global__ __launch_bounds__(1024) void dec_linear_vec_kernel(
    const void* __restrict__ x, const void* __restrict__ w,
    const void* __restrict__ bias, void* __restrict__ out, int B, int K,
    int N) {
  constexpr int H = (ACT == ACT_GLU) ? 2 : 1;
  // K-steps in flight per wave: 48 VGPRs of weights for bf16 — the six
  // steps a wave has at K = 6144 in one trip to memory — and 32 for fp32
  constexpr int U = (BF ? 6 : 2) / H;
  extern __shared__ float part[];  // [nw][H][VEC_BT][TN]

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int nw = blockDim.x >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int n0 = blockIdx.x * TN;
  const int b0 = blockIdx.y * VEC_BT;
  const int nb = min(VEC_BT, B - b0);
  const int ksteps = K / KSTEP;

  long long wrow[H];
  wrow[0] = (long long)(n0 + l15) * K + 16 * l4;
  if constexpr (H == 2) wrow[1] = wrow[0] + (long long)(N >> 1) * K;

  float acc[H][VEC_BT];
#pragma unroll
  for (int h = 0; h < H; ++h)
#pragma unroll
    for (int b = 0; b < VEC_BT; ++b) acc[h][b] = 0.f;

  for (int ks0 = wave; ks0 < ksteps; ks0 += nw * U) {
    raw16<BF> wr[U][H];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int ks = ks0 + u * nw;
      if (ks < ksteps) {
#pragma unroll
        for (int h = 0; h < H; ++h)
          wr[u][h] = ldraw16<BF>(w, wrow[h] + ks * KSTEP);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int ks = ks0 + u * nw;
      if (ks < ksteps) {
        float wv[H][16];
#pragma unroll
        for (int h = 0; h < H; ++h) widen16<BF>(wr[u][h], wv[h]);
#pragma unroll
        for (int b = 0; b < VEC_BT; ++b) {
          if (b < nb) {
            float xv[16];
            ld16<BF>(x, (long long)(b0 + b) * K + ks * KSTEP + 16 * l4, xv);
#pragma unroll
            for (int h = 0; h < H; ++h)
#pragma unroll
              for (int j = 0; j < 16; ++j)
                acc[h][b] = fmaf(wv[h][j], xv[j], acc[h][b]);
          }
        }
      }
    }
  }

  // the four lanes of a row, then the waves through LDS
#pragma unroll
  for (int h = 0; h < H; ++h)
#pragma unroll
    for (int b = 0; b < VEC_BT; ++b) {
      float v = acc[h][b];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      if (lane < 16) part[((wave * H + h) * VEC_BT + b) * TN + l15] = v;
    }
  __syncthreads();

  if (tid < VEC_BT * TN) {
    const int b = tid >> 4, nl = tid & 15;
    if (b < nb)
      epilogue<BF, ACT>(part, nw, H * VEC_BT * TN, VEC_BT * TN, b * TN + nl,
                        bias, out, b0 + b, n0, nl, N);
  }
}

// ---------------------------------------------------------------------------
// mfma path (bf16)
// ---------------------------------------------------------------------------

template <int ACT, int BT>
__global__ __launch_bounds__(1024) void dec_linear_mfma_kernel(
    const short* __restrict__ x, const short* __restrict__ w,
    const short* __restrict__ bias, short* __restrict__ out, int B, int K,
    int N) {
  constexpr int H = (ACT == ACT_GLU) ? 2 : 1;
  // K-steps in flight per wave, 8 VGPRs per fragment pair: 6 steps (96
  // VGPRs) for one half and one batch tile, fewer as the fragments multiply
  constexpr int U = (H + BT == 2) ? 6 : (H + BT == 3) ? 3 : 2;
  extern __shared__ float part[];  // [nw][H][BT][16 batch][TN]

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int nw = blockDim.x >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int n0 = blockIdx.x * TN;
  const int ksteps = K / KSTEP;

  const short* wrow[H];
  wrow[0] = w + (long long)(n0 + l15) * K + 16 * l4;
  if constexpr (H == 2) wrow[1] = wrow[0] + (long long)(N >> 1) * K;
  // lane l feeds batch column l & 15 of its tile; columns >= B get zeros
  const short* xrow[BT];
  bool valid[BT];
#pragma unroll
  for (int t = 0; t < BT; ++t) {
    const int b = t * 16 + l15;
    valid[t] = b < B;
    xrow[t] = x + (long long)(valid[t] ? b : 0) * K + 16 * l4;
  }

  f32x4 acc[H][BT];
#pragma unroll
  for (int h = 0; h < H; ++h)
#pragma unroll
    for (int t = 0; t < BT; ++t) acc[h][t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int ks0 = wave; ks0 < ksteps; ks0 += nw * U) {
    bf16x8 wf[U][H][2], xf[U][BT][2];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int ks = ks0 + u * nw;
      if (ks < ksteps) {
#pragma unroll
        for (int h = 0; h < H; ++h) {
          wf[u][h][0] = *(const bf16x8*)(wrow[h] + ks * KSTEP);
          wf[u][h][1] = *(const bf16x8*)(wrow[h] + ks * KSTEP + 8);
        }
#pragma unroll
        for (int t = 0; t < BT; ++t) {
          xf[u][t][0] = zero;
          xf[u][t][1] = zero;
          if (valid[t]) {
            xf[u][t][0] = *(const bf16x8*)(xrow[t] + ks * KSTEP);
            xf[u][t][1] = *(const bf16x8*)(xrow[t] + ks * KSTEP + 8);
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int ks = ks0 + u * nw;
      if (ks < ksteps) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int h = 0; h < H; ++h)
#pragma unroll
            for (int t = 0; t < BT; ++t)
              acc[h][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  wf[u][h][s], xf[u][t][s], acc[h][t], 0, 0, 0);
      }
    }
  }

  // D: row (weight row) = 4 * (lane >> 4) + r, column (batch) = lane & 15
#pragma unroll
  for (int h = 0; h < H; ++h)
#pragma unroll
    for (int t = 0; t < BT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        part[(((wave * H + h) * BT + t) * 16 + l15) * TN + 4 * l4 + r] =
            acc[h][t][r];
  __syncthreads();

  for (int i = tid; i < BT * 16 * TN; i += blockDim.x) {
    const int b = i >> 4, nl = i & 15;
    if (b < B)
      epilogue<true, ACT>(part, nw, H * BT * 16 * TN, BT * 16 * TN, i, bias,
                          out, b, n0, nl, N);
  }
}

// ---------------------------------------------------------------------------
// launcher
// ---------------------------------------------------------------------------

// waves per workgroup: enough that tiles * waves covers the chip a few times
// over (about 2048 waves), between 4 and 16. Mirrored by the tests' emulation
// of the summation order.
static int waves_for(int tiles) {
  int nw = 4;
  while (nw < 16 && tiles * nw < 2048) nw <<= 1;
  return nw;
}

template <bool BF, int ACT>
static void launch_vec(const void* x, const void* w, const void* bias,
                       void* out, int B, int K, int N, int tiles, int nw,
                       hipStream_t stream) {
  constexpr int H = (ACT == ACT_GLU) ? 2 : 1;
  const dim3 grid(tiles, (B + VEC_BT - 1) / VEC_BT);
  const size_t lds = (size_t)nw * H * VEC_BT * TN * sizeof(float);
  dec_linear_vec_kernel<BF, ACT><<<grid, nw * 64, lds, stream>>>(
      x, w, bias, out, B, K, N);
}

template <int ACT, int BT>
static void launch_mfma(const void* x, const void* w, const void* bias,
                        void* out, int B, int K, int N, int tiles, int nw,
                        hipStream_t stream) {
  constexpr int H = (ACT == ACT_GLU) ? 2 : 1;
  // two halves of two batch tiles: 8 waves keep the partials within 32 KB
  if (H * BT == 4 && nw > 8) nw = 8;
  const size_t lds = (size_t)nw * H * BT * 16 * TN * sizeof(float);
  dec_linear_mfma_kernel<ACT, BT><<<tiles, nw * 64, lds, stream>>>(
      (const short*)x, (const short*)w, (const short*)bias, (short*)out, B, K,
      N);
}

template <int ACT>
static void launch_act(const void* x, const void* w, const void* bias,
                       void* out, int B, int K, int N, bool is_bf16,
                       hipStream_t stream) {
  const int tiles = (ACT == ACT_GLU ? N / 2 : N) / TN;
  const int nw = waves_for(tiles);
  if (!is_bf16)
    launch_vec<false, ACT>(x, w, bias, out, B, K, N, tiles, nw, stream);
  else if (B <= DEC_LINEAR_VEC_MAX_B)
    launch_vec<true, ACT>(x, w, bias, out, B, K, N, tiles, nw, stream);
  else if (B <= 16)
    launch_mfma<ACT, 1>(x, w, bias, out, B, K, N, tiles, nw, stream);
  else
    launch_mfma<ACT, 2>(x, w, bias, out, B, K, N, tiles, nw, stream);
}

extern "C" hipError_t dec_linear_launch(const void* x, const void* w,
                                        const void* bias, void* out, int B,
                                        int K, int N, int act, bool is_bf16,
                                        hipStream_t stream) {
  if (act == ACT_GLU)
    launch_act<ACT_GLU>(x, w, bias, out, B, K, N, is_bf16, stream);
  else if (act == ACT_GELU)
    launch_act<ACT_GELU>(x, w, bias, out, B, K, N, is_bf16, stream);
  else
    launch_act<ACT_NONE>(x, w, bias, out, B, K, N, is_bf16, stream);
  return hipGetLastError();
}
