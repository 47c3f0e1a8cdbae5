// Launcher declaration for the decode linear kernel
// (progen_amd._C_decode_linear). Returns the hipGetLastError() taken right
// after the launch.
#pragma once
#include <hip/hip_runtime.h>

// largest batch the bf16 instantiation serves on the vector-ALU path; above
// it the MFMA path runs (one batch tile up to 16 rows, two up to 32)
#define DEC_LINEAR_VEC_MAX_B 4
#define DEC_LINEAR_MAX_ROWS 32

extern "C" {

// act: 0 none, 1 tanh-GELU, 2 GLU (out is (B, N/2)). ``bias`` may be null.
hipError_t dec_linear_launch(const void* x, const void* w, const void* bias,
                             void* out, int B, int K, int N, int act,
                             bool is_bf16, hipStream_t stream);

}  // extern "C"
