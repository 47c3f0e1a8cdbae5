// Launcher declarations for the decode-step kernels (progen_amd._C_decode).
// Each returns the hipGetLastError() taken right after its launch.
#pragma once
#include <hip/hip_runtime.h>

extern "C" {

hipError_t dec_ln_shift_launch(void* h, const void* res, const void* g,
                               void* prev, void* y, int B, int D, float eps,
                               bool shift, bool is_bf16, hipStream_t stream);

hipError_t dec_attn_launch(const void* qkv, const float* rsin,
                           const float* rcos, const long long* pos,
                           void* k_cache, void* v_cache, void* out, int B,
                           int H, int N, int window, bool is_bf16,
                           hipStream_t stream);

hipError_t dec_sgu_launch(const void* h, const void* g, void* hist,
                          const void* w, const void* bias,
                          const long long* pos, void* out, int B, int N,
                          int d2, float eps, bool is_bf16,
                          hipStream_t stream);

}  // extern "C"
