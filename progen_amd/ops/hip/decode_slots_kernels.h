// Launcher declarations for the slot kernels (progen_amd._C_decode_slots):
// the decode-step kernels with one position per batch row. Each returns the
// hipGetLastError() taken right after its launch. ``pos`` holds B int64
// positions; pos[b] < 0 is an idle row.
#pragma once
#include <hip/hip_runtime.h>

#include "decode_sample_kernels.h"  // DEC_SAMPLE_MIN_V, DEC_SAMPLE_MAX_V

// columns of the sampler's per-row controls
#define DEC_SLOTS_CTL 5  // [len, limit, top_k, seed, stream]

extern "C" {

hipError_t dec_ln_shift_slots_launch(void* h, const void* res, const void* g,
                                     void* prev, void* y, const long long* pos,
                                     int B, int D, float eps, bool shift,
                                     bool is_bf16, hipStream_t stream);

hipError_t dec_attn_slots_launch(const void* qkv, const float* rsin,
                                 const float* rcos, const long long* pos,
                                 void* k_cache, void* v_cache, void* out,
                                 int B, int H, int N, int window, bool is_bf16,
                                 hipStream_t stream);

hipError_t dec_sgu_slots_launch(const void* h, const void* g, void* hist,
                                const void* w, const void* bias,
                                const long long* pos, void* out, int B, int N,
                                int d2, float eps, bool is_bf16,
                                hipStream_t stream);

// ``pos`` is read and written; ``u_out`` may be null. seq (B, L), pads and
// token (B) are int64 and updated in place; ctl is (B, DEC_SLOTS_CTL) int64.
hipError_t dec_sample_slots_launch(const void* logits, long long* pos,
                                   long long* token, long long* seq,
                                   long long* pads, const long long* ctl,
                                   float* u_out, int B, int V, int L,
                                   bool is_bf16, hipStream_t stream);

}  // extern "C"
