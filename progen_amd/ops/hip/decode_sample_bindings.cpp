// PyTorch binding of the decode sampling kernel (progen_amd._C_decode_sample).
//
// A fourth extension module beside progen_amd._C, progen_amd._C_decode and
// progen_amd._C_decode_linear, whose export lists are pinned: one entry
// point, the sampler of the cached decode step (decode_sample.hip). It
// follows the launch contract of checks.h: dtype, shape/contiguity,
// divisibility, range and device checks in that order, then DeviceScope and
// LAUNCH. Nothing is allocated: every output is an argument updated in place.
//
// ``pos`` is a 0-dim int64 DEVICE tensor, as for the other decode kernels,
// and ``seed`` a (1,) one, so that a captured graph reads both at replay.
// Their values cannot be checked here without a device read; the kernel
// returns without touching memory when pos + 1 is outside [1, L).

#include <torch/extension.h>

#include "checks.h"
#include "decode_sample_kernels.h"

using namespace chk;

// Next token of every row from logits (B, V): argmax when ``greedy``, else
// gumbel-max over the strict top-k (top_k = 0: the whole row) with noise
// from Philox4x32-10 keyed by ``seed`` at counter (j / 4, pos + 1, b, 0).
// seq (B, L), pads (B) and token (B) are updated in place; ``u_out`` (B, V)
// fp32, when given, receives the uniform draws.
void dec_sample(const at::Tensor& logits, const at::Tensor& pos,
                const at::Tensor& seed, at::Tensor seq, const at::Tensor& lens,
                at::Tensor pads, at::Tensor token, int64_t top_k, bool greedy,
                const c10::optional<at::Tensor>& u_out) {
  const char* op = "dec_sample";
  const bool bf = dtype_bf16_or_fp32(op, ARG(logits));
  dtype_is(op, ARG(pos), at::kLong);
  dtype_is(op, ARG(seed), at::kLong);
  dtype_is(op, ARG(seq), at::kLong);
  dtype_is(op, ARG(lens), at::kLong);
  dtype_is(op, ARG(pads), at::kLong);
  dtype_is(op, ARG(token), at::kLong);
  if (u_out) dtype_is(op, Arg{"u_out", *u_out}, at::kFloat);
  contiguous_rank(op, ARG(logits), 2);
  const int64_t B = logits.size(0), V = logits.size(1);
  contiguous_rank(op, ARG(pos), 0);
  contiguous_shape(op, ARG(seed), {1});
  contiguous_rank(op, ARG(seq), 2);
  const int64_t L = seq.size(1);
  contiguous_shape(op, ARG(seq), {B, L});
  contiguous_shape(op, ARG(lens), {B});
  contiguous_shape(op, ARG(pads), {B});
  contiguous_shape(op, ARG(token), {B});
  if (u_out) contiguous_shape(op, Arg{"u_out", *u_out}, {B, V});
  const int Bi = extent_int(op, "B", B, kGridYZ);
  CHK(V >= DEC_SAMPLE_MIN_V && V <= DEC_SAMPLE_MAX_V, op, "V", V,
      "must be in [", DEC_SAMPLE_MIN_V, ", ", DEC_SAMPLE_MAX_V, "]");
  const int Li = extent_int(op, "L", L);
  CHK(top_k >= 0 && top_k <= V, op, "top_k", top_k, "must be in [0, ", V, "]");
  same_gpu(op, {ARG(logits), ARG(pos), ARG(seed), ARG(seq), ARG(lens),
                ARG(pads), ARG(token)});
  if (u_out) same_gpu(op, {ARG(logits), Arg{"u_out", *u_out}});

  DeviceScope dev(logits);
  LAUNCH(op, dec_sample_launch(
                 logits.data_ptr(), (const long long*)pos.data_ptr<int64_t>(),
                 (const long long*)seed.data_ptr<int64_t>(),
                 (long long*)seq.data_ptr<int64_t>(),
                 (const long long*)lens.data_ptr<int64_t>(),
                 (long long*)pads.data_ptr<int64_t>(),
                 (long long*)token.data_ptr<int64_t>(),
                 u_out ? u_out->data_ptr<float>() : nullptr, Bi, (int)V, Li,
                 (int)top_k, greedy, bf, dev.stream));
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("dec_sample", &dec_sample,
        "decode step: greedy or top-k gumbel-max token per row, in place",
        py::arg("logits"), py::arg("pos"), py::arg("seed"), py::arg("seq"),
        py::arg("lens"), py::arg("pads"), py::arg("token"), py::arg("top_k"),
        py::arg("greedy"), py::arg("u_out") = py::none());
}
