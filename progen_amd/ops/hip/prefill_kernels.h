// Launcher declarations for the prefill kernels (progen_amd._C_prefill).
// Each returns the hipGetLastError() taken right after its launch.
#pragma once
#include <hip/hip_runtime.h>

extern "C" {

// qkv, qkv_rot (B, Np, 3*H*64) bf16; rsin/rcos fp32 with at least Np rows of
// 64; k_cache/v_cache (B, H, Nc, 64) bf16, rows [0, P) written.
hipError_t prefill_rope_kv_launch(const void* qkv, const float* rsin,
                                  const float* rcos, void* qkv_rot,
                                  void* k_cache, void* v_cache, int B, int Np,
                                  int H, int Nc, int P, hipStream_t stream);

// x (B, Np, 2*d2) bf16, g (d2), gate_ln (B, Np, d2), hist (B, Nc, d2) with
// rows [0, P) written. R = B * Np rows.
hipError_t prefill_gate_ln_launch(const void* x, const void* g, void* gate_ln,
                                  void* hist, int R, int Np, int Nc, int d2,
                                  int P, float eps, hipStream_t stream);

// The same two with the cache row and the row count read from device memory
// (prefill_admit.hip): admit (R, 2) int64 = [slot, rows] per batch row; the
// caches have S rows, and batch row r writes rows [0, min(rows, P)) of cache
// row ``slot`` when 0 <= slot < S, else nothing.
hipError_t admit_rope_kv_launch(const void* qkv, const float* rsin,
                                const float* rcos, void* qkv_rot,
                                void* k_cache, void* v_cache,
                                const long long* admit, int R, int Np, int H,
                                int Nc, int S, int P, hipStream_t stream);

// rows = R * Np.
hipError_t admit_gate_ln_launch(const void* x, const void* g, void* gate_ln,
                                void* hist, const long long* admit, int rows,
                                int Np, int Nc, int d2, int S, int P, float eps,
                                hipStream_t stream);

}  // extern "C"
