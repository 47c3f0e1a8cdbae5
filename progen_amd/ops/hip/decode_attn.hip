// Decode-step attention row: rotary on q, k AND v at row ``pos``, the cache
// write, and one softmax(q K^T) V row over the local band, per (batch, head).
//
//   band = cache rows [max(0, w0 - window), pos],  w0 = (pos / window) * window
//
// While pos < window the full forward's zero lookback window is part of the
// band: ``window`` keys that are all zero and unmasked, i.e. ``window``
// logits of exactly 0 in the softmax max and denominator with zero values.
//
// One 256-thread workgroup per (b, h). A key row is 64 elements = 8 chunks
// of 8, so 8 consecutive lanes hold one row and the block's 32 lane groups
// take band rows start + g, start + g + 32, ...  K and V go from global
// memory straight to registers. Every group keeps its own running
// (max, sum, acc[8]); the groups of a wave are combined with shuffles and
// the four waves once through LDS. Row ``pos`` itself is never loaded:
// group 0 holds the rotated k and v in registers, writes them to the cache
// and adds their term. Rows before the band and after ``pos`` are never
// read. ``pos`` is read from device memory; outside [0, N) the block
// returns before it touches qkv, the caches or out. The body is in
// decode_attn_body.h, shared with the slot kernel.

#include "common.h"
#include "decode_attn_body.h"
#include "decode_kernels.h"

template <bool BF>
__global__ __launch_bounds__(256) void dec_attn_kernel(
    const void* __restrict__ qkv, const float* __restrict__ rsin,
    const float* __restrict__ rcos, const long long* __restrict__ pos_ptr,
    void* k_cache, void* v_cache, void* __restrict__ out, int H, int N,
    int window) {
  dec_attn_body<BF, false>(qkv, rsin, rcos, pos_ptr, k_cache, v_cache, out, H,
                           N, window);
}

extern "C" hipError_t dec_attn_launch(const void* qkv, const float* rsin,
                                      const float* rcos, const long long* pos,
                                      void* k_cache, void* v_cache, void* out,
                                      int B, int H, int N, int window,
                                      bool is_bf16, hipStream_t stream) {
  if (is_bf16)
    dec_attn_kernel<true><<<B * H, 256, 0, stream>>>(
        qkv, rsin, rcos, pos, k_cache, v_cache, out, H, N, window);
  else
    dec_attn_kernel<false><<<B * H, 256, 0, stream>>>(
        qkv, rsin, rcos, pos, k_cache, v_cache, out, H, N, window);
  return hipGetLastError();
}
