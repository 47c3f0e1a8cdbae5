// The prefill kernels for a captured graph (progen_amd/engine.py, prefill at
// admission): prefill.hip's two kernels with the cache row and the row count
// of every batch row read from device memory, so that one captured forward
// over static (R, Np) token buffers can fill any slot of an S-row cache with
// any number of rows.
//
//   admit_rope_kv   prefill_rope_kv with admit (R, 2) int64 = [slot, rows]
//   admit_gate_ln   prefill_gate_ln with the same tensor
//
// Batch row r stores its rows n < min(rows, P) into cache row ``slot`` when
// 0 <= slot < S, and nothing otherwise: the host cannot see the values, so
// the range guard is in the kernel (prefill_body.h). P stays the host's
// upper bound. The full-sequence outputs are written for every row, with
// prefill.hip's bits: the bodies are the same source.

#include "common.h"
#include "prefill_body.h"
#include "prefill_kernels.h"

__global__ __launch_bounds__(256) void admit_rope_kv_kernel(
    const short* __restrict__ qkv,  // (R, Np, 3*H*DH) bf16
    const float* __restrict__ rsin, const float* __restrict__ rcos,
    short* __restrict__ qkv_rot,
    short* __restrict__ k_cache,  // (S, H, Nc, DH) bf16
    short* __restrict__ v_cache, const long long* __restrict__ admit, int R,
    int N, int H, int Nc, int S, int P) {
  prefill_rope_kv_body<true>(qkv, rsin, rcos, qkv_rot, k_cache, v_cache, admit,
                             R, N, H, Nc, S, P);
}

__global__ __launch_bounds__(LN_BLOCK) void admit_gate_ln_kernel(
    const void* __restrict__ x_,  // (R, Np, 2*d2) bf16
    const void* __restrict__ g_, void* __restrict__ y_,  // (R, Np, d2)
    void* __restrict__ hist_,                            // (S, Nc, d2)
    const long long* __restrict__ admit, int N, int Nc, int Dv, int S, int P,
    float eps) {
  __shared__ float red[LN_WAVES];
  if (Dv <= LN_BLOCK)
    prefill_gate_ln_body<true, true>(x_, g_, y_, hist_, admit, N, Nc, Dv, S, P,
                                     eps, red);
  else
    prefill_gate_ln_body<true, false>(x_, g_, y_, hist_, admit, N, Nc, Dv, S,
                                      P, eps, red);
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

extern "C" {

hipError_t admit_rope_kv_launch(const void* qkv, const float* rsin,
                                const float* rcos, void* qkv_rot,
                                void* k_cache, void* v_cache,
                                const long long* admit, int R, int Np, int H,
                                int Nc, int S, int P, hipStream_t stream) {
  int gx = (3 * H * (DH / 8) + 255) / 256;
  long long bn = (long long)R * Np;
  int gy = (int)(bn < 2048 ? bn : 2048);
  dim3 grid(gx, gy);
  admit_rope_kv_kernel<<<grid, 256, 0, stream>>>(
      (const short*)qkv, rsin, rcos, (short*)qkv_rot, (short*)k_cache,
      (short*)v_cache, admit, R, Np, H, Nc, S, P);
  return hipGetLastError();
}

hipError_t admit_gate_ln_launch(const void* x, const void* g, void* gate_ln,
                                void* hist, const long long* admit, int rows,
                                int Np, int Nc, int d2, int S, int P, float eps,
                                hipStream_t stream) {
  admit_gate_ln_kernel<<<rows, LN_BLOCK, 0, stream>>>(
      x, g, gate_ln, hist, admit, Np, Nc, d2 / 8, S, P, eps);
  return hipGetLastError();
}

}  // extern "C"
