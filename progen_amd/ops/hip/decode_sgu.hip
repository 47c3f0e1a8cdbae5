// Decode-step spatial gating row (gMLP SGU) per batch element:
//
//   gl           = LN(gate) * g            h = [xa | gate], each d2 wide
//   hist[b, pos] <- gl
//   out          = xa * (sum_{n <= pos} w[pos, n] * hist[b, n] + bias[pos])
//
// Grid: (d2 / 64 column tiles) x B, 256 threads. The gate row is a few KB,
// so every workgroup recomputes its LN statistics rather than wait for
// another one. A workgroup writes only its own 64 columns of hist[b, pos]
// and takes the n = pos term from registers, so nothing written in this
// launch is read in it. A 64-column slice of a hist row is 8 chunks of 8:
// 8 consecutive lanes hold one row slice and the block's 32 lane groups
// take rows g, g + 32, ... below pos, straight from global memory to
// registers; rows above pos are never read. ``pos`` is read from device
// memory; outside [0, N) the block returns before it touches h, hist or out.
// The body is in decode_sgu_body.h, shared with the slot kernel.

#include "common.h"
#include "decode_kernels.h"
#include "decode_sgu_body.h"

#define TILE DEC_SGU_TILE

template <bool BF>
__global__ __launch_bounds__(256) void dec_sgu_kernel(
    const void* __restrict__ h, const void* __restrict__ g, void* hist,
    const void* __restrict__ w, const void* __restrict__ bias,
    const long long* __restrict__ pos_ptr, void* __restrict__ out, int N,
    int d2, float eps) {
  dec_sgu_body<BF, false>(h, g, hist, w, bias, pos_ptr, out, N, d2, eps);
}

extern "C" hipError_t dec_sgu_launch(const void* h, const void* g, void* hist,
                                     const void* w, const void* bias,
                                     const long long* pos, void* out, int B,
                                     int N, int d2, float eps, bool is_bf16,
                                     hipStream_t stream) {
  const dim3 grid(d2 / TILE, B);
  if (is_bf16)
    dec_sgu_kernel<true><<<grid, 256, 0, stream>>>(h, g, hist, w, bias, pos,
                                                   out, N, d2, eps);
  else
    dec_sgu_kernel<false><<<grid, 256, 0, stream>>>(h, g, hist, w, bias, pos,
                                                    out, N, d2, eps);
  return hipGetLastError();
}
