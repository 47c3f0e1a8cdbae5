// PyTorch binding of the prefill kernels (progen_amd._C_prefill).
//
// A fifth extension module beside progen_amd._C, progen_amd._C_decode,
// progen_amd._C_decode_linear and progen_amd._C_decode_sample, whose export
// lists are pinned: the two kernels that fill the decode caches from one
// full-sequence forward over the prime (prefill.hip). Both follow the launch
// contract of checks.h: dtype, shape/contiguity, divisibility, range and
// device checks in that order, then DeviceScope, allocation and LAUNCH.
//
// ``P``, the number of cache rows to fill, is a host scalar: prefill runs
// eagerly, before any graph is captured. The caches are updated in place.
//
// Both take one trailing optional ``admit``, a (B, 2) int64 device tensor of
// [slot, rows] per batch row, for the captured prefill of progen_amd/engine.py
// (prefill_admit.hip): the caches may then have any number S >= 1 of rows,
// batch row b fills rows [0, min(rows, P)) of cache row ``slot`` when
// 0 <= slot < S and nothing otherwise, and ``P`` is only the host's upper
// bound. The values are on the device, so their range is the kernel's to
// guard. Without it every check, message and launch is as before.

#include <torch/extension.h>

#include <algorithm>

#include "checks.h"
#include "prefill_kernels.h"

using namespace chk;

// rope_qkv's rotation of qkv (B, Np, 3*H*64); the rotated k and v of rows
// n < P are also stored head-major into k_cache/v_cache (B, H, Nc, 64).
// Returns qkv_rot, for attn_fwd.
at::Tensor prefill_rope_kv(const at::Tensor& qkv, const at::Tensor& sin,
                           const at::Tensor& cos, at::Tensor k_cache,
                           at::Tensor v_cache, int64_t P,
                           const c10::optional<at::Tensor>& admit) {
  const char* op = "prefill_rope_kv";
  const bool adm = admit.has_value();
  dtype_is(op, ARG(qkv), at::kBFloat16);
  dtype_is(op, ARG(sin), at::kFloat);
  dtype_is(op, ARG(cos), at::kFloat);
  dtype_same(op, ARG(k_cache), ARG(qkv));
  dtype_same(op, ARG(v_cache), ARG(qkv));
  if (adm) dtype_is(op, Arg{"admit", *admit}, at::kLong);
  contiguous_rank(op, ARG(qkv), 3);
  const int64_t B = qkv.size(0), Np = qkv.size(1), C = qkv.size(2);
  rope_table(op, ARG(sin), Np);
  rope_table(op, ARG(cos), Np);
  contiguous_rank(op, ARG(k_cache), 4);
  const int64_t Nc = k_cache.size(2);
  const int64_t S = adm ? k_cache.size(0) : B;  // cache rows
  if (adm) contiguous_shape(op, Arg{"admit", *admit}, {B, 2});
  multiple_of(op, "qkv.size(2)", C, 3 * 64);  // (q|k|v) x heads x 64
  const int64_t heads = C / (3 * 64);
  contiguous_shape(op, ARG(k_cache), {S, heads, Nc, 64});
  contiguous_shape(op, ARG(v_cache), {S, heads, Nc, 64});
  const int Bi = extent_int(op, "B", B), Ni = extent_int(op, "Np", Np);
  const int Si = extent_int(op, "S", S);
  const int H = extent_int(op, "heads", heads);
  const int Nci = extent_int(op, "Nc", Nc);
  const int Pi = extent_int(op, "P", P, std::min(Np, Nc));
  same_gpu(op, {ARG(qkv), ARG(sin), ARG(cos), ARG(k_cache), ARG(v_cache)});
  if (adm) same_gpu(op, {ARG(qkv), Arg{"admit", *admit}});

  DeviceScope dev(qkv);
  auto qkv_rot = at::empty_like(qkv);
  if (adm) {
    LAUNCH(op, admit_rope_kv_launch(
                   qkv.data_ptr(), sin.data_ptr<float>(), cos.data_ptr<float>(),
                   qkv_rot.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                   (const long long*)admit->data_ptr<int64_t>(), Bi, Ni, H, Nci,
                   Si, Pi, dev.stream));
    return qkv_rot;
  }
  LAUNCH(op, prefill_rope_kv_launch(
                 qkv.data_ptr(), sin.data_ptr<float>(), cos.data_ptr<float>(),
                 qkv_rot.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), Bi,
                 Ni, H, Nci, Pi, dev.stream));
  return qkv_rot;
}

// Scale-only LN of the gate half x[..., d2:] of x (B, Np, 2*d2), read in
// place; rows n < P are also stored into hist (B, Nc, d2). Returns gate_ln
// (B, Np, d2), for sgu_fwd.
at::Tensor prefill_gate_ln(const at::Tensor& x, const at::Tensor& norm_weight,
                           at::Tensor hist, int64_t P, double eps,
                           const c10::optional<at::Tensor>& admit) {
  const char* op = "prefill_gate_ln";
  const bool adm = admit.has_value();
  dtype_is(op, ARG(x), at::kBFloat16);
  dtype_same(op, ARG(norm_weight), ARG(x));
  dtype_same(op, ARG(hist), ARG(x));
  if (adm) dtype_is(op, Arg{"admit", *admit}, at::kLong);
  contiguous_rank(op, ARG(x), 3);
  const int64_t B = x.size(0), Np = x.size(1), C = x.size(2);
  contiguous_rank(op, ARG(hist), 3);
  const int64_t Nc = hist.size(1);
  const int64_t S = adm ? hist.size(0) : B;  // cache rows
  if (adm) contiguous_shape(op, Arg{"admit", *admit}, {B, 2});
  // both halves are rows of whole 64-element chunks, as sgu_fwd wants them
  multiple_of(op, "x.size(2)", C, 2 * 64);
  const int64_t d2 = C / 2;
  contiguous_numel(op, ARG(norm_weight), d2);
  contiguous_shape(op, ARG(hist), {S, Nc, d2});
  const int Ni = extent_int(op, "Np", Np), D = extent_int(op, "d2", d2);
  const int Nci = extent_int(op, "Nc", Nc);
  const int R = extent_int(op, "B*Np", B * Np);
  const int Si = extent_int(op, "S", S);
  const int Pi = extent_int(op, "P", P, std::min(Np, Nc));
  same_gpu(op, {ARG(x), ARG(norm_weight), ARG(hist)});
  if (adm) same_gpu(op, {ARG(x), Arg{"admit", *admit}});

  DeviceScope dev(x);
  auto gate_ln = at::empty({B, Np, d2}, x.options());
  if (adm) {
    LAUNCH(op, admit_gate_ln_launch(
                   x.data_ptr(), norm_weight.data_ptr(), gate_ln.data_ptr(),
                   hist.data_ptr(),
                   (const long long*)admit->data_ptr<int64_t>(), R, Ni, Nci, D,
                   Si, Pi, (float)eps, dev.stream));
    return gate_ln;
  }
  LAUNCH(op, prefill_gate_ln_launch(x.data_ptr(), norm_weight.data_ptr(),
                                    gate_ln.data_ptr(), hist.data_ptr(), R, Ni,
                                    Nci, D, Pi, (float)eps, dev.stream));
  return gate_ln;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("prefill_rope_kv", &prefill_rope_kv,
        "prefill: rotary on q, k, v + k/v cache rows [0, P)", py::arg("qkv"),
        py::arg("sin"), py::arg("cos"), py::arg("k_cache"),
        py::arg("v_cache"), py::arg("P"), py::arg("admit") = py::none());
  m.def("prefill_gate_ln", &prefill_gate_ln,
        "prefill: LN of the SGU gate half + gate history rows [0, P)",
        py::arg("x"), py::arg("norm_weight"), py::arg("hist"), py::arg("P"),
        py::arg("eps") = 1e-5, py::arg("admit") = py::none());
}
