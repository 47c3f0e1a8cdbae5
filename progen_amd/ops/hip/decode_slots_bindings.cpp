// PyTorch bindings for the slot kernels (progen_amd._C_decode_slots).
//
// The decode-step kernels with one position per batch row (decode_slots.hip),
// for a decode batch whose rows serve different requests
// (progen_amd/engine.py). The checked entries of the three kernels shared
// with the scalar step are in decode_entries.h; the functions here are its
// SLOTS = true instances. The sampler's entry is this file's own and follows
// the launch contract of checks.h: dtype, shape/contiguity, divisibility,
// range and device checks in that order, then DeviceScope and LAUNCH.
//
// ``pos`` is a (B,) int64 DEVICE tensor; pos[b] < 0 marks an idle row. Its
// values, like those of the sampler's ``ctl``, cannot be checked here without
// a device read: the kernels treat a position outside [0, N) as idle, and the
// sampler retires a row whose next position is outside [1, min(limit, L)).

#include <torch/extension.h>

#include "decode_entries.h"

using namespace chk;

// dec_ln_shift with a position per row: an idle row gets a zero y and keeps
// its h and prev; a row at position 0 shifts in zeros instead of prev.
at::Tensor dec_ln_shift_slots(at::Tensor h,
                              const c10::optional<at::Tensor>& res,
                              const at::Tensor& g,
                              const c10::optional<at::Tensor>& prev,
                              const at::Tensor& pos, bool shift, double eps) {
  return dec::ln_shift<true>("dec_ln_shift_slots", h, res, g, prev, &pos,
                             shift, eps);
}

// dec_attn with a position per row: rotary, cache write and band at pos[b];
// an idle row gets a zero out row and keeps its caches.
at::Tensor dec_attn_slots(const at::Tensor& qkv, const at::Tensor& rsin,
                          const at::Tensor& rcos, const at::Tensor& pos,
                          at::Tensor k_cache, at::Tensor v_cache,
                          int64_t window) {
  return dec::attn<true>("dec_attn_slots", qkv, rsin, rcos, pos, k_cache,
                         v_cache, window);
}

// dec_sgu with a position per row: history write and causal row at pos[b];
// an idle row gets a zero out row and keeps its history.
at::Tensor dec_sgu_slots(const at::Tensor& h, const at::Tensor& g,
                         at::Tensor hist, const at::Tensor& w,
                         const at::Tensor& bias, const at::Tensor& pos,
                         double eps) {
  return dec::sgu<true>("dec_sgu_slots", h, g, hist, w, bias, pos, eps);
}

// dec_sample with a position and a control row [len, limit, top_k, seed,
// stream] per batch row. pos (B), token (B), seq (B, L) and pads (B) are
// updated in place: a row that sampled position w moves to pos[b] = w, or to
// -1 once it has two pads or w + 1 reached its limit. ``u_out`` (B, V) fp32,
// when given, receives the uniform draws of the rows that drew any.
void dec_sample_slots(const at::Tensor& logits, at::Tensor pos,
                      at::Tensor token, at::Tensor seq, at::Tensor pads,
                      const at::Tensor& ctl,
                      const c10::optional<at::Tensor>& u_out) {
  const char* op = "dec_sample_slots";
  const bool bf = dtype_bf16_or_fp32(op, ARG(logits));
  dtype_is(op, ARG(pos), at::kLong);
  dtype_is(op, ARG(token), at::kLong);
  dtype_is(op, ARG(seq), at::kLong);
  dtype_is(op, ARG(pads), at::kLong);
  dtype_is(op, ARG(ctl), at::kLong);
  if (u_out) dtype_is(op, Arg{"u_out", *u_out}, at::kFloat);
  contiguous_rank(op, ARG(logits), 2);
  const int64_t B = logits.size(0), V = logits.size(1);
  contiguous_shape(op, ARG(pos), {B});
  contiguous_shape(op, ARG(token), {B});
  contiguous_rank(op, ARG(seq), 2);
  const int64_t L = seq.size(1);
  contiguous_shape(op, ARG(seq), {B, L});
  contiguous_shape(op, ARG(pads), {B});
  contiguous_shape(op, ARG(ctl), {B, DEC_SLOTS_CTL});
  if (u_out) contiguous_shape(op, Arg{"u_out", *u_out}, {B, V});
  const int Bi = extent_int(op, "B", B, kGridYZ);
  CHK(V >= DEC_SAMPLE_MIN_V && V <= DEC_SAMPLE_MAX_V, op, "V", V,
      "must be in [", DEC_SAMPLE_MIN_V, ", ", DEC_SAMPLE_MAX_V, "]");
  const int Li = extent_int(op, "L", L);
  same_gpu(op, {ARG(logits), ARG(pos), ARG(token), ARG(seq), ARG(pads),
                ARG(ctl)});
  if (u_out) same_gpu(op, {ARG(logits), Arg{"u_out", *u_out}});

  DeviceScope dev(logits);
  LAUNCH(op, dec_sample_slots_launch(
                 logits.data_ptr(), (long long*)pos.data_ptr<int64_t>(),
                 (long long*)token.data_ptr<int64_t>(),
                 (long long*)seq.data_ptr<int64_t>(),
                 (long long*)pads.data_ptr<int64_t>(),
                 (const long long*)ctl.data_ptr<int64_t>(),
                 u_out ? u_out->data_ptr<float>() : nullptr, Bi, (int)V, Li,
                 bf, dev.stream));
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("dec_ln_shift_slots", &dec_ln_shift_slots,
        "slot decode step: residual add + LN + token shift, position per row",
        py::arg("h"), py::arg("res"), py::arg("g"), py::arg("prev"),
        py::arg("pos"), py::arg("shift"), py::arg("eps") = 1e-5);
  m.def("dec_attn_slots", &dec_attn_slots,
        "slot decode step: rotary + cache write + one local attention row",
        py::arg("qkv"), py::arg("rsin"), py::arg("rcos"), py::arg("pos"),
        py::arg("k_cache"), py::arg("v_cache"), py::arg("window"));
  m.def("dec_sgu_slots", &dec_sgu_slots,
        "slot decode step: gate LN + history write + causal spatial row",
        py::arg("h"), py::arg("g"), py::arg("hist"), py::arg("w"),
        py::arg("bias"), py::arg("pos"), py::arg("eps") = 1e-5);
  m.def("dec_sample_slots", &dec_sample_slots,
        "slot decode step: per-row token, position advance and retirement",
        py::arg("logits"), py::arg("pos"), py::arg("token"), py::arg("seq"),
        py::arg("pads"), py::arg("ctl"), py::arg("u_out") = py::none());
}
