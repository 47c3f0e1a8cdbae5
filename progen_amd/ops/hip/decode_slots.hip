// The decode-step kernels with one position per batch row, for a decode
// batch whose rows ("slots") serve different requests (progen_amd/engine.py).
//
// Each kernel is the body of its scalar twin (decode_*_body.h) instantiated
// with SLOTS = true: ``pos`` holds B int64 positions and workgroups of batch
// row b read pos[b]. A row with pos[b] < 0 is idle: its workgroups touch no
// cache, prev, hist, seq, pads or token; the three forward kernels write the
// row of their output as zeros, so nothing uninitialised reaches the GEMMs
// that follow. Rows are independent as in the scalar kernels: no atomics, no
// workgroup waits on another, and every early return is uniform over the
// workgroup and comes before any barrier. Grids and block sizes are those of
// the scalar kernels.
//
//   dec_ln_shift_slots  a row at position 0 reads its shifted half as zeros:
//                       the slot's prev row belongs to the request before it
//   dec_attn_slots      rotary, band and cache write at pos[b]
//   dec_sgu_slots       history write and causal row at pos[b]
//   dec_sample_slots    per-row len, limit, top_k, seed and stream; advances
//                       pos[b] or retires the row (pos[b] <- -1)

#include "common.h"
#include "decode_attn_body.h"
#include "decode_ln_shift_body.h"
#include "decode_sample_body.h"
#include "decode_sgu_body.h"
#include "decode_slots_kernels.h"

template <bool BF, bool ONE>
__global__ __launch_bounds__(256) void dec_ln_shift_slots_kernel(
    void* h, const void* __restrict__ res, const void* __restrict__ g,
    void* prev, void* __restrict__ y, const long long* __restrict__ pos, int D,
    float eps, bool shift) {
  dec_ln_shift_body<BF, ONE, true>(h, res, g, prev, y, pos, D, eps, shift);
}

template <bool BF>
__global__ __launch_bounds__(256) void dec_attn_slots_kernel(
    const void* __restrict__ qkv, const float* __restrict__ rsin,
    const float* __restrict__ rcos, const long long* __restrict__ pos,
    void* k_cache, void* v_cache, void* __restrict__ out, int H, int N,
    int window) {
  dec_attn_body<BF, true>(qkv, rsin, rcos, pos, k_cache, v_cache, out, H, N,
                          window);
}

template <bool BF>
__global__ __launch_bounds__(256) void dec_sgu_slots_kernel(
    const void* __restrict__ h, const void* __restrict__ g, void* hist,
    const void* __restrict__ w, const void* __restrict__ bias,
    const long long* __restrict__ pos, void* __restrict__ out, int N, int d2,
    float eps) {
  dec_sgu_body<BF, true>(h, g, hist, w, bias, pos, out, N, d2, eps);
}

template <bool BF>
__global__ __launch_bounds__(256) void dec_sample_slots_kernel(
    const void* __restrict__ logits, long long* pos, long long* token,
    long long* seq, long long* pads, const long long* __restrict__ ctl,
    float* __restrict__ u_out, int V, int L) {
  dec_sample_body<BF, true>(logits, pos, nullptr, seq, nullptr, pads, token,
                            u_out, ctl, pos, V, L, 0, false);
}

extern "C" hipError_t dec_ln_shift_slots_launch(
    void* h, const void* res, const void* g, void* prev, void* y,
    const long long* pos, int B, int D, float eps, bool shift, bool is_bf16,
    hipStream_t stream) {
#define GO(BF, ONE)                                                        \
  dec_ln_shift_slots_kernel<BF, ONE><<<B, 256, 0, stream>>>(h, res, g, prev, \
                                                            y, pos, D, eps,  \
                                                            shift)
  const bool one = D <= 2048;
  if (is_bf16) {
    if (one) GO(true, true); else GO(true, false);
  } else {
    if (one) GO(false, true); else GO(false, false);
  }
#undef GO
  return hipGetLastError();
}

extern "C" hipError_t dec_attn_slots_launch(
    const void* qkv, const float* rsin, const float* rcos,
    const long long* pos, void* k_cache, void* v_cache, void* out, int B,
    int H, int N, int window, bool is_bf16, hipStream_t stream) {
  if (is_bf16)
    dec_attn_slots_kernel<true><<<B * H, 256, 0, stream>>>(
        qkv, rsin, rcos, pos, k_cache, v_cache, out, H, N, window);
  else
    dec_attn_slots_kernel<false><<<B * H, 256, 0, stream>>>(
        qkv, rsin, rcos, pos, k_cache, v_cache, out, H, N, window);
  return hipGetLastError();
}

extern "C" hipError_t dec_sgu_slots_launch(const void* h, const void* g,
                                           void* hist, const void* w,
                                           const void* bias,
                                           const long long* pos, void* out,
                                           int B, int N, int d2, float eps,
                                           bool is_bf16, hipStream_t stream) {
  const dim3 grid(d2 / DEC_SGU_TILE, B);
  if (is_bf16)
    dec_sgu_slots_kernel<true><<<grid, 256, 0, stream>>>(h, g, hist, w, bias,
                                                         pos, out, N, d2, eps);
  else
    dec_sgu_slots_kernel<false><<<grid, 256, 0, stream>>>(
        h, g, hist, w, bias, pos, out, N, d2, eps);
  return hipGetLastError();
}

extern "C" hipError_t dec_sample_slots_launch(
    const void* logits, long long* pos, long long* token, long long* seq,
    long long* pads, const long long* ctl, float* u_out, int B, int V, int L,
    bool is_bf16, hipStream_t stream) {
  if (is_bf16)
    dec_sample_slots_kernel<true><<<B, 256, 0, stream>>>(
        logits, pos, token, seq, pads, ctl, u_out, V, L);
  else
    dec_sample_slots_kernel<false><<<B, 256, 0, stream>>>(
        logits, pos, token, seq, pads, ctl, u_out, V, L);
  return hipGetLastError();
}
