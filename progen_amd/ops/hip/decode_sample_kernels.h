// Launcher declaration for the decode sampling kernel
// (progen_amd._C_decode_sample). Returns the hipGetLastError() taken right
// after the launch.
#pragma once
#include <hip/hip_runtime.h>

// one workgroup of 256 threads stages a whole row and owns four vocabulary
// entries (one Philox block) per thread
#define DEC_SAMPLE_MIN_V 2
#define DEC_SAMPLE_MAX_V 1024

extern "C" {

// top_k: 0 = no top-k mask. ``u_out`` may be null. seq (B, L), lens, pads
// and token (B) are int64 and updated in place.
hipError_t dec_sample_launch(const void* logits, const long long* pos,
                             const long long* seed, long long* seq,
                             const long long* lens, long long* pads,
                             long long* token, float* u_out, int B, int V,
                             int L, int top_k, bool greedy, bool is_bf16,
                             hipStream_t stream);

}  // extern "C"
