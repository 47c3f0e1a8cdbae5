// The checked entry points of the three decode kernels that exist both with a
// scalar position (progen_amd._C_decode, decode_bindings.cpp) and with one
// position per batch row (progen_amd._C_decode_slots,
// decode_slots_bindings.cpp). Host only.
//
// One launch contract per kernel, as the decode_*_body.h headers hold one
// device body per kernel: the two steps differ in the shape of ``pos`` (0-dim
// or (B,)), for the LN in whether it takes ``pos`` at all, and in the launcher
// called. SLOTS selects all three at compile time, so each module refers only
// to the launchers it links. Checks follow checks.h: dtype, shape/contiguity,
// divisibility, range and device in that order, then DeviceScope, allocation
// and LAUNCH.
#pragma once

#include <torch/extension.h>

#include "checks.h"
#include "decode_kernels.h"
#include "decode_slots_kernels.h"

namespace dec {

using namespace chk;

// ``pos`` is a 0-dim int64 tensor for the scalar step, (B,) for the slot step
template <bool SLOTS>
inline void pos_shape(const char* op, Arg pos, int64_t B) {
  if constexpr (SLOTS) {
    contiguous_shape(op, pos, {B});
  } else {
    contiguous_rank(op, pos, 0);
  }
}

// Residual add + scale-only LN + token shift on one row per batch element.
// ``h`` (B, D) and ``prev`` (B, D) are updated in place; returns y. The slot
// step passes its ``pos``; the scalar step has none and passes nullptr.
template <bool SLOTS>
at::Tensor ln_shift(const char* op, at::Tensor h,
                    const c10::optional<at::Tensor>& res, const at::Tensor& g,
                    const c10::optional<at::Tensor>& prev,
                    const at::Tensor* pos, bool shift, double eps) {
  const bool bf = dtype_bf16_or_fp32(op, ARG(h));
  if (res) dtype_same(op, Arg{"res", *res}, ARG(h));
  dtype_same(op, ARG(g), ARG(h));
  if (prev) dtype_same(op, Arg{"prev", *prev}, ARG(h));
  if constexpr (SLOTS) dtype_is(op, Arg{"pos", *pos}, at::kLong);
  contiguous_rank(op, ARG(h), 2);
  const int64_t B = h.size(0), D = h.size(1);
  if (res) contiguous_shape(op, Arg{"res", *res}, h.sizes());
  contiguous_numel(op, ARG(g), D);
  if (prev) contiguous_shape(op, Arg{"prev", *prev}, h.sizes());
  if constexpr (SLOTS) contiguous_shape(op, Arg{"pos", *pos}, {B});
  CHK(prev.has_value() || !shift, op, "prev", "None", "must be given when shift is set");
  // the shifted half D/2 must be whole 8-element chunks
  multiple_of(op, "D", D, 16);
  const int Bi = extent_int(op, "B", B, kGridYZ);
  const int Di = extent_int(op, "D", D);
  if constexpr (SLOTS) {
    same_gpu(op, {ARG(h), ARG(g), Arg{"pos", *pos}});
  } else {
    same_gpu(op, {ARG(h), ARG(g)});
  }
  if (res) same_gpu(op, {ARG(h), Arg{"res", *res}});
  if (prev) same_gpu(op, {ARG(h), Arg{"prev", *prev}});

  DeviceScope dev(h);
  auto y = at::empty_like(h);
  void* hp = h.data_ptr();
  const void* rp = res ? res->data_ptr() : nullptr;
  void* pp = prev ? prev->data_ptr() : nullptr;
  if constexpr (SLOTS) {
    LAUNCH(op, dec_ln_shift_slots_launch(
                   hp, rp, g.data_ptr(), pp, y.data_ptr(),
                   (const long long*)pos->data_ptr<int64_t>(), Bi, Di,
                   (float)eps, shift, bf, dev.stream));
  } else {
    LAUNCH(op, dec_ln_shift_launch(hp, rp, g.data_ptr(), pp, y.data_ptr(), Bi,
                                   Di, (float)eps, shift, bf, dev.stream));
  }
  return y;
}

// Rotary at row ``pos`` on q, k and v, cache write, one attention row per
// (batch, head). dim_head is fixed at 64; the caches (B, H, N, 64) are
// updated in place; returns out (B, H*64).
template <bool SLOTS>
at::Tensor attn(const char* op, const at::Tensor& qkv, const at::Tensor& rsin,
                const at::Tensor& rcos, const at::Tensor& pos,
                at::Tensor k_cache, at::Tensor v_cache, int64_t window) {
  const int wsz = extent_int(op, "window", window);
  const bool bf = dtype_bf16_or_fp32(op, ARG(qkv));
  dtype_is(op, ARG(rsin), at::kFloat);
  dtype_is(op, ARG(rcos), at::kFloat);
  dtype_is(op, ARG(pos), at::kLong);
  dtype_same(op, ARG(k_cache), ARG(qkv));
  dtype_same(op, ARG(v_cache), ARG(qkv));
  contiguous_rank(op, ARG(k_cache), 4);
  const int64_t B = k_cache.size(0), H = k_cache.size(1), N = k_cache.size(2);
  CHK(k_cache.size(3) == 64, op, "k_cache", k_cache.sizes(),
      "must have shape (B, H, N, 64)");
  contiguous_shape(op, ARG(v_cache), k_cache.sizes());
  contiguous_shape(op, ARG(qkv), {B, 3 * H * 64});
  rope_table(op, ARG(rsin), N);
  rope_table(op, ARG(rcos), N);
  pos_shape<SLOTS>(op, ARG(pos), B);
  multiple_of(op, "window", window, 64);
  multiple_of(op, "N", N, window);
  const int BH = extent_int(op, "B*H", B * H, kGridYZ);
  const int Ni = extent_int(op, "N", N);
  same_gpu(op, {ARG(qkv), ARG(rsin), ARG(rcos), ARG(pos), ARG(k_cache),
                ARG(v_cache)});

  DeviceScope dev(qkv);
  auto out = at::empty({B, H * 64}, qkv.options());
  const auto launch = [] {
    if constexpr (SLOTS) return dec_attn_slots_launch;
    else return dec_attn_launch;
  }();
  LAUNCH(op, launch(qkv.data_ptr(), rsin.data_ptr<float>(),
                    rcos.data_ptr<float>(),
                    (const long long*)pos.data_ptr<int64_t>(),
                    k_cache.data_ptr(), v_cache.data_ptr(), out.data_ptr(),
                    BH / (int)H, (int)H, Ni, wsz, bf, dev.stream));
  return out;
}

// LN of the gate half, history write and the causal spatial row of the
// SGU. ``h`` is (B, 2*d2) = [xa | gate]; ``hist`` (B, N, d2) is updated in
// place; returns out (B, d2).
template <bool SLOTS>
at::Tensor sgu(const char* op, const at::Tensor& h, const at::Tensor& g,
               at::Tensor hist, const at::Tensor& w, const at::Tensor& bias,
               const at::Tensor& pos, double eps) {
  const bool bf = dtype_bf16_or_fp32(op, ARG(h));
  dtype_same(op, ARG(g), ARG(h));
  dtype_same(op, ARG(hist), ARG(h));
  dtype_same(op, ARG(w), ARG(h));
  dtype_same(op, ARG(bias), ARG(h));
  dtype_is(op, ARG(pos), at::kLong);
  contiguous_rank(op, ARG(hist), 3);
  const int64_t B = hist.size(0), N = hist.size(1), d2 = hist.size(2);
  contiguous_shape(op, ARG(h), {B, 2 * d2});
  contiguous_numel(op, ARG(g), d2);
  contiguous_shape(op, ARG(w), {N, N});
  contiguous_shape(op, ARG(bias), {N, 1});
  pos_shape<SLOTS>(op, ARG(pos), B);
  multiple_of(op, "d2", d2, 64);  // one workgroup per 64-column tile
  const int Bi = extent_int(op, "B", B, kGridYZ);
  const int Ni = extent_int(op, "N", N);
  const int d2i = extent_int(op, "d2", d2);
  same_gpu(op, {ARG(h), ARG(g), ARG(hist), ARG(w), ARG(bias), ARG(pos)});

  DeviceScope dev(h);
  auto out = at::empty({B, d2}, h.options());
  const auto launch = [] {
    if constexpr (SLOTS) return dec_sgu_slots_launch;
    else return dec_sgu_launch;
  }();
  LAUNCH(op, launch(h.data_ptr(), g.data_ptr(), hist.data_ptr(), w.data_ptr(),
                    bias.data_ptr(), (const long long*)pos.data_ptr<int64_t>(),
                    out.data_ptr(), Bi, Ni, d2i, (float)eps, bf, dev.stream));
  return out;
}

}  // namespace dec
