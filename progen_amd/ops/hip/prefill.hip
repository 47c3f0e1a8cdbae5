// Prefill of the decode caches from one full-sequence forward over the prime
// (progen_amd/decode.py, prefill): the two places where the full forward
// computes, for every row at once, what a decode step stores for its own row.
// Both are memory-bound row kernels that write their full-sequence output as
// before and, for rows n < P, the same 16 B vectors into the cache as well:
//
//   prefill_rope_kv   rope_qkv.hip's rotation; the rotated k and v also go
//                     head-major into the (B, H, Nc, 64) k/v caches;
//   prefill_gate_ln   scale-only LN of the SGU gate half, read in place out
//                     of the (B, Np, 2*d2) activation; the LN'd rows also go
//                     into the (B, Nc, d2) gate history.
//
// P is a host scalar: prefill runs eagerly, before any graph is captured.
// Cache rows >= P are never written.

#include "common.h"
#include "prefill_body.h"
#include "prefill_kernels.h"

// The bodies are prefill_body.h's, shared with prefill_admit.hip, which reads
// the cache row and the row count from device memory instead.

__global__ __launch_bounds__(256) void prefill_rope_kv_kernel(
    const short* __restrict__ qkv,  // (B, Np, 3*H*DH) bf16
    const float* __restrict__ rsin, const float* __restrict__ rcos,
    short* __restrict__ qkv_rot,
    short* __restrict__ k_cache,  // (B, H, Nc, DH) bf16
    short* __restrict__ v_cache, int B, int N, int H, int Nc, int P) {
  prefill_rope_kv_body<false>(qkv, rsin, rcos, qkv_rot, k_cache, v_cache,
                              nullptr, B, N, H, Nc, B, P);
}

__global__ __launch_bounds__(LN_BLOCK) void prefill_gate_ln_kernel(
    const void* __restrict__ x_,  // (B, Np, 2*d2) bf16
    const void* __restrict__ g_, void* __restrict__ y_,  // (B, Np, d2)
    void* __restrict__ hist_,                            // (B, Nc, d2)
    int N, int Nc, int Dv, int P, float eps) {
  __shared__ float red[LN_WAVES];
  if (Dv <= LN_BLOCK)
    prefill_gate_ln_body<false, true>(x_, g_, y_, hist_, nullptr, N, Nc, Dv, 0,
                                      P, eps, red);
  else
    prefill_gate_ln_body<false, false>(x_, g_, y_, hist_, nullptr, N, Nc, Dv,
                                       0, P, eps, red);
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

extern "C" {

hipError_t prefill_rope_kv_launch(const void* qkv, const float* rsin,
                                  const float* rcos, void* qkv_rot,
                                  void* k_cache, void* v_cache, int B, int Np,
                                  int H, int Nc, int P, hipStream_t stream) {
  int gx = (3 * H * (DH / 8) + 255) / 256;
  long long bn = (long long)B * Np;
  int gy = (int)(bn < 2048 ? bn : 2048);
  dim3 grid(gx, gy);
  prefill_rope_kv_kernel<<<grid, 256, 0, stream>>>(
      (const short*)qkv, rsin, rcos, (short*)qkv_rot, (short*)k_cache,
      (short*)v_cache, B, Np, H, Nc, P);
  return hipGetLastError();
}

hipError_t prefill_gate_ln_launch(const void* x, const void* g, void* gate_ln,
                                  void* hist, int R, int Np, int Nc, int d2,
                                  int P, float eps, hipStream_t stream) {
  prefill_gate_ln_kernel<<<R, LN_BLOCK, 0, stream>>>(x, g, gate_ln, hist, Np,
                                                     Nc, d2 / 8, P, eps);
  return hipGetLastError();
}

}  // extern "C"
