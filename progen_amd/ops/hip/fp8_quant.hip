// Fused e4m3 quantization kernels for the fp8 GEMM path (ops/fp8.py).
//
// tools/bench_fp8.py measured the hipBLASLt e4m3 GEMMs at 1.77-2.06x
// bf16 — and the eager quantization chain (float() copy, div, clamp,
// to(float8): 4 full passes with an fp32 intermediate) eating the
// entire gain. These kernels make quantization ONE pass each:
//
//   quant_e4m3:   bf16 -> e4m3 at a device-scalar scale, clamped to
//                 +-448 in registers (no separate clamp pass);
//   quant_e4m3_t: (N, K) bf16 row-major -> (K, N) e4m3 row-major
//                 (the column-major operand torch._scaled_mm needs for
//                 the dgrad) through 64x64 LDS tiles — both the global
//                 read and the global write stay coalesced.
//
// Scales stay on device (graph-capturable; no host sync).

#include "common.h"

#define QBLOCK 256

// x / scale clamped to the e4m3 range. On gfx950 v_cvt_pk_fp8_f32 rounds
// up to 464 to 448 but turns anything larger into the NaN byte 0x7f, so
// the clamp is not optional: a value beyond 448 * scale (a stale scale)
// must saturate as clamp(-448, 448).to(float8_e4m3fn) does.
__device__ __forceinline__ float q_scaled(short b, float inv) {
  return fminf(fmaxf(bf2f(b) * inv, -448.0f), 448.0f);
}

__global__ __launch_bounds__(QBLOCK) void quant_e4m3_kernel(
    const short* __restrict__ in, unsigned char* __restrict__ out,
    const float* __restrict__ scale, long long n8) {
  const float inv = 1.0f / *scale;
  for (long long i = blockIdx.x * (long long)QBLOCK + threadIdx.x; i < n8;
       i += (long long)gridDim.x * QBLOCK) {
    bf16x8 v = ((const bf16x8*)in)[i];
    unsigned short b01, b23, b45, b67;
    // v_cvt_pk_fp8_f32 packs two fp32 into two e4m3 bytes (RNE)
    b01 = (unsigned short)__builtin_amdgcn_cvt_pk_fp8_f32(
        q_scaled(((short*)&v)[0], inv), q_scaled(((short*)&v)[1], inv), 0, false);
    b23 = (unsigned short)__builtin_amdgcn_cvt_pk_fp8_f32(
        q_scaled(((short*)&v)[2], inv), q_scaled(((short*)&v)[3], inv), 0, false);
    b45 = (unsigned short)__builtin_amdgcn_cvt_pk_fp8_f32(
        q_scaled(((short*)&v)[4], inv), q_scaled(((short*)&v)[5], inv), 0, false);
    b67 = (unsigned short)__builtin_amdgcn_cvt_pk_fp8_f32(
        q_scaled(((short*)&v)[6], inv), q_scaled(((short*)&v)[7], inv), 0, false);
    unsigned long long packed = (unsigned long long)b01 |
                                ((unsigned long long)b23 << 16) |
                                ((unsigned long long)b45 << 32) |
                                ((unsigned long long)b67 << 48);
    ((unsigned long long*)out)[i] = packed;
  }
}

// 64x64 tile transpose-quantize: block = 256 threads; each loads 16
// rows x 64 cols bf16 (4 passes), stages through LDS with a +1-element
// row pad (65*2 B rows) to dodge bank conflicts on the transposed read.
#define TT 64

__global__ __launch_bounds__(QBLOCK) void quant_e4m3_t_kernel(
    const short* __restrict__ in,  // (N, K) bf16 row-major
    unsigned char* __restrict__ out,  // (K, N) e4m3 row-major
    const float* __restrict__ scale, int Nr, int Kc) {
  __shared__ float tile[TT][TT + 1];
  const float inv = 1.0f / *scale;
  const int tiles_k = (Kc + TT - 1) / TT;
  for (int tid = blockIdx.x; ; tid += gridDim.x) {
    const int tn = tid / tiles_k;
    const int tk = tid % tiles_k;
    if (tn * TT >= Nr) break;
    const int n0 = tn * TT, k0 = tk * TT;
    // load 64x64 (row-major, coalesced 2-B... 4 rows per pass of 256)
    for (int p = 0; p < TT * TT / QBLOCK; ++p) {
      const int idx = p * QBLOCK + threadIdx.x;
      const int r = idx / TT, c = idx % TT;
      const int n = n0 + r, k = k0 + c;
      tile[r][c] = (n < Nr && k < Kc)
          ? q_scaled(in[(long long)n * Kc + k], inv) : 0.f;
    }
    __syncthreads();
    // write transposed: out row = k, col = n (coalesced over n)
    for (int p = 0; p < TT * TT / QBLOCK; ++p) {
      const int idx = p * QBLOCK + threadIdx.x;
      const int r = idx / TT, c = idx % TT;   // r -> k, c -> n
      const int k = k0 + r, n = n0 + c;
      if (k < Kc && n < Nr && (c & 1) == 0) {
        unsigned short b = (unsigned short)__builtin_amdgcn_cvt_pk_fp8_f32(
            tile[c][r], tile[c + 1][r], 0, false);
        *(unsigned short*)(out + (long long)k * Nr + n) = b;
      }
    }
    __syncthreads();
  }
}

extern "C" {

hipError_t quant_e4m3_launch(const void* in, void* out, const float* scale,
                             long long numel, hipStream_t stream) {
  long long n8 = numel / 8;
  int grid = (int)((n8 + QBLOCK - 1) / QBLOCK);
  if (grid > 4096) grid = 4096;
  quant_e4m3_kernel<<<grid, QBLOCK, 0, stream>>>(
      (const short*)in, (unsigned char*)out, scale, n8);
  return hipGetLastError();
}

hipError_t quant_e4m3_t_launch(const void* in, void* out, const float* scale,
                               int Nr, int Kc, hipStream_t stream) {
  int tiles = ((Nr + TT - 1) / TT) * ((Kc + TT - 1) / TT);
  int grid = tiles < 4096 ? tiles : 4096;
  quant_e4m3_t_kernel<<<grid, QBLOCK, 0, stream>>>(
      (const short*)in, (unsigned char*)out, scale, Nr, Kc);
  return hipGetLastError();
}

}  // extern "C"
