// Common device helpers for ProGen CDNA4 (gfx950) kernels.
// Wavefront = 64; block sizes are multiples of 64 throughout.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#define WAVE 64

using bf16 = __hip_bfloat16;

// vector types for wide loads (16 B / lane sweet spot)
typedef short bf16x8 __attribute__((ext_vector_type(8)));   // 8 bf16 = 16 B
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float bf2f(short u) {
  union { unsigned int i; float f; } c;
  c.i = ((unsigned int)(unsigned short)u) << 16;
  return c.f;
}

__device__ __forceinline__ short f2bf(float f) {
  // __float2bfloat16 lowers to ONE v_cvt_pk_bf16_f32 (RNE, same
  // rounding as torch); the manual bit-math RNE this replaces was
  // three VALU ops in every kernel's store path
  __hip_bfloat16 b = __float2bfloat16(f);
  return *(short*)&b;
}

// wave-wide reductions (64 lanes)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// reduce across a 16-lane subgroup (xor over lanes 1,2,4,8); used where the
// MFMA C-layout spreads one output row over lanes sharing (lane & 15)
__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ float group16_max(float v) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// fast tanh on v_exp_f32 (libm tanhf is a slow ocml polynomial — the
// round-2 profile put glu_bwd at 56% of HBM peak purely on VALU cost;
// v_exp is ~2 cycles beside other work). (e-1)/(e+1) with the argument
// clamped so exp never overflows to inf (inf/inf = NaN); |x| >= 15 is
// tanh = +-1 to beyond fp32 precision anyway.
__device__ __forceinline__ float fast_tanh(float x) {
  float xc = fminf(fmaxf(x, -15.0f), 15.0f);
  float e = __expf(2.0f * xc);
  return (e - 1.0f) / (e + 1.0f);
}

// tanh-approximation GELU (matches jax.nn.gelu approximate=True and
// torch F.gelu(approximate="tanh"))
__device__ __forceinline__ float gelu_tanh(float x) {
  const float k0 = 0.7978845608028654f;  // sqrt(2/pi)
  const float k1 = 0.044715f;
  float inner = k0 * (x + k1 * x * x * x);
  return 0.5f * x * (1.0f + fast_tanh(inner));
}

__device__ __forceinline__ float gelu_tanh_grad(float x) {
  const float k0 = 0.7978845608028654f;
  const float k1 = 0.044715f;
  float x2 = x * x;
  float inner = k0 * (x + k1 * x * x2);
  float t = fast_tanh(inner);
  float dinner = k0 * (1.0f + 3.0f * k1 * x2);
  return 0.5f * (1.0f + t) + 0.5f * x * (1.0f - t * t) * dinner;
}

// value AND derivative from ONE tanh (the backward needs both; two
// separate calls were the other half of glu_bwd's VALU bill)
__device__ __forceinline__ void gelu_tanh_both(float x, float* val,
                                               float* grad) {
  const float k0 = 0.7978845608028654f;
  const float k1 = 0.044715f;
  float x2 = x * x;
  float inner = k0 * (x + k1 * x * x2);
  float t = fast_tanh(inner);
  float dinner = k0 * (1.0f + 3.0f * k1 * x2);
  *val = 0.5f * x * (1.0f + t);
  *grad = 0.5f * (1.0f + t) + 0.5f * x * (1.0f - t * t) * dinner;
}

// 8 consecutive elements as fp32, for kernels instantiated on both storage
// types: one 16 B load for bf16, two for fp32. ``idx`` is an element index
// and a multiple of 8, so every access is 16 B aligned.
template <bool BF>
__device__ __forceinline__ void ld8(const void* p, long long idx, float* x) {
  if constexpr (BF) {
    const bf16x8 v = *(const bf16x8*)((const short*)p + idx);
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = bf2f(v[j]);
  } else {
    const f32x4 a = *(const f32x4*)((const float*)p + idx);
    const f32x4 b = *(const f32x4*)((const float*)p + idx + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[j] = a[j];
      x[j + 4] = b[j];
    }
  }
}

template <bool BF>
__device__ __forceinline__ void st8(void* p, long long idx, const float* x) {
  if constexpr (BF) {
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = f2bf(x[j]);
    *(bf16x8*)((short*)p + idx) = v;
  } else {
    f32x4 a, b;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a[j] = x[j];
      b[j] = x[j + 4];
    }
    *(f32x4*)((float*)p + idx) = a;
    *(f32x4*)((float*)p + idx + 4) = b;
  }
}

// one element of the storage type, and the value an fp32 result takes once
// it has been stored in that type
template <bool BF>
__device__ __forceinline__ float ld1(const void* p, long long idx) {
  if constexpr (BF) return bf2f(((const short*)p)[idx]);
  else return ((const float*)p)[idx];
}

template <bool BF>
__device__ __forceinline__ void st1(void* p, long long idx, float v) {
  if constexpr (BF) ((short*)p)[idx] = f2bf(v);
  else ((float*)p)[idx] = v;
}

template <bool BF>
__device__ __forceinline__ float round_trip(float x) {
  if constexpr (BF) return bf2f(f2bf(x));
  else return x;
}

// The 16 B vector of a storage type, for kernels in which one thread owns one
// 16 B load: 8 bf16 or FOUR fp32. (ld8 hands a thread 8 elements of either
// type; which elements a thread owns fixes the order of every sum it feeds,
// so a kernel stays with the one it was written on.) vget/vset read and
// write element j as fp32; vset rounds to the storage type.
template <bool BF>
struct vec16 {
  using type = f32x4;
  static constexpr int N = 4;
};
template <>
struct vec16<true> {
  using type = bf16x8;
  static constexpr int N = 8;
};
template <bool BF>
using vec16_t = typename vec16<BF>::type;

template <bool BF>
__device__ __forceinline__ float vget(const vec16_t<BF>& v, int j) {
  if constexpr (BF) return bf2f(v[j]);
  else return v[j];
}

template <bool BF>
__device__ __forceinline__ void vset(vec16_t<BF>& v, int j, float x) {
  if constexpr (BF) v[j] = f2bf(x);
  else v[j] = x;
}

// A vector a kernel has just stored, made opaque to the compiler before its
// elements are read back into a sum OF THE STORED VALUES (bias_grad.hip). Left
// to itself the compiler folds the product behind an fp32 element into the
// running sum as an fma, so that the sum is not of what was stored, and, with
// the elements' second use in sight, contracts and pairs the arithmetic before
// the store differently from the kernel without the sum: glu_bwd's fp32 dh
// differed in the last bit between the two.
template <typename VEC>
__device__ __forceinline__ void opaque_vec(VEC& v) {
  asm volatile("" : "+v"(v));
}

// sum over a 256-thread block, result in every thread. ``red`` holds 4
// floats of LDS; consecutive calls must use different arrays.
__device__ __forceinline__ float block256_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}
