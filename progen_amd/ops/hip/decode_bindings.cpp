// PyTorch bindings for the decode-step kernels (progen_amd._C_decode).
//
// The three fused kernels that replace every non-GEMM op of the cached
// decode step (progen_amd/decode.py, forward_step_fused). Their checked
// entries are in decode_entries.h, shared with the slot step
// (decode_slots_bindings.cpp); the functions here are its SLOTS = false
// instances under the names and signatures this module exports.
//
// ``pos`` is a 0-dim int64 DEVICE tensor so that a captured graph can
// advance it between replays. Its value cannot be checked here without a
// device read; the kernels return without touching memory when it is
// outside [0, N).

#include <torch/extension.h>

#include "decode_entries.h"

at::Tensor dec_ln_shift(at::Tensor h, const c10::optional<at::Tensor>& res,
                        const at::Tensor& g,
                        const c10::optional<at::Tensor>& prev, bool shift,
                        double eps) {
  return dec::ln_shift<false>("dec_ln_shift", h, res, g, prev, nullptr, shift,
                              eps);
}

at::Tensor dec_attn(const at::Tensor& qkv, const at::Tensor& rsin,
                    const at::Tensor& rcos, const at::Tensor& pos,
                    at::Tensor k_cache, at::Tensor v_cache, int64_t window) {
  return dec::attn<false>("dec_attn", qkv, rsin, rcos, pos, k_cache, v_cache,
                          window);
}

at::Tensor dec_sgu(const at::Tensor& h, const at::Tensor& g, at::Tensor hist,
                   const at::Tensor& w, const at::Tensor& bias,
                   const at::Tensor& pos, double eps) {
  return dec::sgu<false>("dec_sgu", h, g, hist, w, bias, pos, eps);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("dec_ln_shift", &dec_ln_shift,
        "decode step: residual add + LN + token shift on one row");
  m.def("dec_attn", &dec_attn,
        "decode step: rotary + cache write + one local attention row");
  m.def("dec_sgu", &dec_sgu,
        "decode step: gate LN + history write + causal spatial row");
}
