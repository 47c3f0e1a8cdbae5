// Bodies of the two prefill kernels, written once for prefill.hip (the cache
// row and the row count come from the host) and for prefill_admit.hip (both
// are read from device memory), as decode_*_body.h does for the slot kernels.
//
// ADMIT = false: batch row b fills cache row b, rows n < P. ``admit`` and
//                ``S`` are not read.
// ADMIT = true:  batch row b reads admit[b] = [slot, rows] and fills cache
//                row ``slot`` of an S-row cache, rows n < min(rows, P), when
//                0 <= slot < S; any other slot, or rows <= 0, stores nothing
//                of that batch row into a cache. P is the host's upper bound
//                min(Np, Nc) at most, so the guard keeps every store inside
//                the cache whatever the device values are. Two batch rows
//                that name one slot would race: the caller names each once.
//
// The full-sequence outputs are written for every row in both modes. The
// arithmetic is the same source in both, under the compiler's default
// contraction, which is what rope_qkv.hip's rotation is compiled with: the
// instruction counts of the instantiations are compared in
// profiles/engine_prefill.md.
#pragma once

#include "common.h"

#define DH 64

// ---------------------------------------------------------------------------
// rope + k/v cache write
// ---------------------------------------------------------------------------
// The rotation is rope_qkv_kernel's, expression for expression, so that
// qkv_rot has its bits. Thread order too: grid.x covers one (b, n) row's
// 3H*8 vector units contiguously and grid.y stripes the rows (rope_qkv.hip
// measured the scattered alternative 23% slower). The 8 lanes of a head slot
// then hold one rotated 64-element head row, which is one contiguous 128 B
// cache row.
template <bool ADMIT>
__device__ __forceinline__ void prefill_rope_kv_body(
    const short* __restrict__ qkv,  // (B, Np, 3*H*DH) bf16
    const float* __restrict__ rsin, const float* __restrict__ rcos,
    short* __restrict__ qkv_rot,
    short* __restrict__ k_cache,  // (B or S, H, Nc, DH) bf16
    short* __restrict__ v_cache,
    const long long* __restrict__ admit,  // (B, 2) [slot, rows]
    int B, int N, int H, int Nc, int S, int P) {
  const long long HD3 = 3LL * H * DH;
  const int u = blockIdx.x * 256 + (int)threadIdx.x;
  if (u >= 3 * H * (DH / 8)) return;
  const int hslot = u >> 3;
  const int g = u & 7;
  const int d0 = g * 8;
  // slots [0, H) are q, [H, 2H) k, [2H, 3H) v
  short* const cache = hslot < H ? nullptr : (hslot < 2 * H ? k_cache : v_cache);
  const int head = hslot < 2 * H ? hslot - H : hslot - 2 * H;
  const long long BN = (long long)B * N;
  for (long long bn = blockIdx.y; bn < BN; bn += gridDim.y) {
    const int n = (int)(bn % N);

    const long long off = bn * HD3 + (long long)hslot * DH + d0;
    bf16x8 v = *(const bf16x8*)(qkv + off);
    float x[8], sv[8], cv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = bf2f(((short*)&v)[j]);
    *(f32x4*)(sv) = *(const f32x4*)(rsin + (long long)n * DH + d0);
    *(f32x4*)(sv + 4) = *(const f32x4*)(rsin + (long long)n * DH + d0 + 4);
    *(f32x4*)(cv) = *(const f32x4*)(rcos + (long long)n * DH + d0);
    *(f32x4*)(cv + 4) = *(const f32x4*)(rcos + (long long)n * DH + d0 + 4);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      float x0 = x[2 * p], x1 = x[2 * p + 1];
      float s = sv[2 * p], c = cv[2 * p];
      x[2 * p] = x0 * c - x1 * s;
      x[2 * p + 1] = x1 * c + x0 * s;
    }
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) ((short*)&o)[j] = f2bf(x[j]);
    *(bf16x8*)(qkv_rot + off) = o;
    if (ADMIT) {
      if (cache != nullptr && n < P) {
        const long long b = bn / N;
        const long long slot = admit[2 * b], rows = admit[2 * b + 1];
        if (slot >= 0 && slot < S && n < rows)
          *(bf16x8*)(cache + ((slot * H + head) * Nc + n) * DH + d0) = o;
      }
    } else {
      if (cache != nullptr && n < P) {
        const long long b = bn / N;
        *(bf16x8*)(cache + ((b * H + head) * Nc + n) * DH + d0) = o;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// gate LN + history write
// ---------------------------------------------------------------------------
// ln_shift_fwd_kernel's row body (ln_shift.hip) without shift, residual and
// saved statistics: one block per row, 16 B per lane, fp32 statistics with
// the centred second moment, ONE (the row's vectors stay in registers, Dv <=
// LN_BLOCK) or !ONE (a thread re-reads its vectors in every pass) picked once
// per block. The input row is the second half of a 2*d2 wide row.
#define LN_BLOCK 256
#define LN_WAVES (LN_BLOCK / WAVE)

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

template <bool ADMIT, bool ONE>
__device__ __forceinline__ void prefill_gate_ln_body(
    const void* __restrict__ x_,  // (B, Np, 2*d2) bf16
    const void* __restrict__ g_, void* __restrict__ y_,  // (B, Np, d2)
    void* __restrict__ hist_,                            // (B or S, Nc, d2)
    const long long* __restrict__ admit,                 // (B, 2) [slot, rows]
    int N, int Nc, int Dv, int S, int P, float eps, float* red) {
  constexpr bool BF = true;
  using VEC = vec16_t<BF>;
  constexpr int VLEN = vec16<BF>::N;
  const VEC *x = (const VEC*)x_, *g = (const VEC*)g_;
  VEC *y = (VEC*)y_, *hist = (VEC*)hist_;
  const int row = blockIdx.x;
  const int n = row % N;
  const long long in = (long long)row * 2 * Dv + Dv;  // the gate half
  const long long out = (long long)row * Dv;
  // block-uniform: the cache row this block also writes, if any
  bool store = n < P;
  long long crow = row / N;
  if (ADMIT) {
    const long long slot = admit[2 * crow], rows = admit[2 * crow + 1];
    store = store && slot >= 0 && slot < S && n < rows;
    crow = slot;
  }
  const long long hrow = (crow * Nc + n) * Dv;
  const int D = Dv * VLEN;

  VEC v;
  float s = 0.f;
  for (int i = threadIdx.x; i < Dv; i += LN_BLOCK) {
    v = x[in + i];
#pragma unroll
    for (int j = 0; j < VLEN; ++j) s += vget<BF>(v, j);
    if (ONE) break;
  }
  const float mu = ln_block_sum(s, red) / D;

  float ss = 0.f;
  for (int i = threadIdx.x; i < Dv; i += LN_BLOCK) {
    if (!ONE) v = x[in + i];
#pragma unroll
    for (int j = 0; j < VLEN; ++j) {
      const float c = vget<BF>(v, j) - mu;
      ss += c * c;
    }
    if (ONE) break;
  }
  const float var = ln_block_sum(ss, red) / D;
  const float rs = rsqrtf(var + eps);

  for (int i = threadIdx.x; i < Dv; i += LN_BLOCK) {
    if (!ONE) v = x[in + i];
    const VEC gw = g[i];
    VEC o;
#pragma unroll
    for (int j = 0; j < VLEN; ++j)
      vset<BF>(o, j, (vget<BF>(v, j) - mu) * rs * vget<BF>(gw, j));
    y[out + i] = o;
    if (store) hist[hrow + i] = o;
    if (ONE) break;
  }
}
