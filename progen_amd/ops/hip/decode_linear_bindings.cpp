// PyTorch binding of the decode linear kernel (progen_amd._C_decode_linear).
//
// A third extension module beside progen_amd._C and progen_amd._C_decode,
// whose export lists are pinned: one entry point, the linear op of the
// cached decode step with its bias and activation folded in
// (decode_linear.hip). It follows the launch contract of checks.h: dtype,
// shape/contiguity, divisibility, range and device checks in that order,
// then DeviceScope, allocation and LAUNCH.

#include <torch/extension.h>

#include <string>

#include "checks.h"
#include "decode_linear_kernels.h"

using namespace chk;

// out (B, N') = act(x (B, K) @ w (N, K)^T + bias (N)); act is "none",
// "gelu" (N' = N) or "glu" (N' = N/2, value half times gelu of gate half).
at::Tensor dec_linear(const at::Tensor& x, const at::Tensor& w,
                      const c10::optional<at::Tensor>& bias,
                      const std::string& act) {
  const char* op = "dec_linear";
  const int acti = act == "none" ? 0 : act == "gelu" ? 1 : act == "glu" ? 2 : -1;
  CHK(acti >= 0, op, "act", act, "must be one of none, gelu, glu");
  const bool bf = dtype_bf16_or_fp32(op, ARG(x));
  dtype_same(op, ARG(w), ARG(x));
  if (bias) dtype_same(op, Arg{"bias", *bias}, ARG(x));
  contiguous_rank(op, ARG(x), 2);
  contiguous_rank(op, ARG(w), 2);
  const int64_t B = x.size(0), K = x.size(1), N = w.size(0);
  contiguous_shape(op, ARG(w), {N, K});
  if (bias) contiguous_numel(op, Arg{"bias", *bias}, N);
  // a wave step is 64 K elements; a workgroup owns 16 columns (GLU: of
  // each half)
  multiple_of(op, "K", K, 64);
  multiple_of(op, "N", N, acti == 2 ? 32 : 16);
  const int Bi = extent_int(op, "B", B, DEC_LINEAR_MAX_ROWS);
  const int Ki = extent_int(op, "K", K);
  const int Ni = extent_int(op, "N", N);
  same_gpu(op, {ARG(x), ARG(w)});
  if (bias) same_gpu(op, {ARG(x), Arg{"bias", *bias}});

  DeviceScope dev(x);
  auto out = at::empty({B, acti == 2 ? N / 2 : N}, x.options());
  LAUNCH(op, dec_linear_launch(x.data_ptr(), w.data_ptr(),
                               bias ? bias->data_ptr() : nullptr,
                               out.data_ptr(), Bi, Ki, Ni, acti, bf,
                               dev.stream));
  return out;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("dec_linear", &dec_linear,
        "decode step: linear + bias + none/GELU/GLU epilogue for 1..32 rows");
}
