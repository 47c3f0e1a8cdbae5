// Argument checks shared by every entry point in bindings.cpp.
//
// Each failure raises "<op>: <argument> <what was expected>, got <what it
// was>". An entry point runs its checks in one fixed order — dtype, then
// shape/contiguity/relations, then divisibility, then range, then device —
// and only afterwards takes the device guard, allocates and launches.
// Device comes last so everything above it can be exercised with CPU
// tensors; nothing is dereferenced before it passes. No check does device
// work (no sync, no copy, no allocation).
#pragma once

#include <torch/extension.h>

#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <hip/hip_runtime.h>

#include <climits>
#include <initializer_list>

namespace chk {

// a tensor argument together with the name it is reported under
struct Arg {
  const char* name;
  const at::Tensor& t;
};
#define ARG(t) chk::Arg{#t, t}

// the one message format; TORCH_CHECK builds the text only on failure
// (``got`` precedes the variadic pieces of the expectation)
#define CHK(cond, op, what, got, ...) \
  TORCH_CHECK(cond, op, ": ", what, " ", __VA_ARGS__, ", got ", got)

constexpr int64_t kGridYZ = 65535;  // HIP limit on grid y and z extents

// ---- 1. dtype -------------------------------------------------------------

inline void dtype_is(const char* op, Arg a, at::ScalarType want) {
  CHK(a.t.scalar_type() == want, op, a.name, a.t.scalar_type(),
      "must have dtype ", want);
}

// the kernels instantiated for both 16 B vector types; true for bf16
inline bool dtype_bf16_or_fp32(const char* op, Arg a) {
  const auto st = a.t.scalar_type();
  CHK(st == at::kBFloat16 || st == at::kFloat, op, a.name, st,
      "must have dtype BFloat16 or Float");
  return st == at::kBFloat16;
}

// tensors a kernel reads with one vector type share a dtype
inline void dtype_same(const char* op, Arg a, Arg ref) {
  CHK(a.t.scalar_type() == ref.t.scalar_type(), op, a.name,
      a.t.scalar_type(), "must have ", ref.name, "'s dtype ",
      ref.t.scalar_type());
}

// ---- 2. rank, shape, contiguity -------------------------------------------

inline void contiguous(const char* op, Arg a) {
  CHK(a.t.is_contiguous(), op, a.name, c10::str("strides ", a.t.strides()),
      "must be contiguous");
}

inline void contiguous_rank(const char* op, Arg a, int64_t rank) {
  CHK(a.t.dim() == rank, op, a.name, a.t.dim(), "must have ", rank, " dims");
  contiguous(op, a);
}

inline void contiguous_shape(const char* op, Arg a, at::IntArrayRef want) {
  CHK(a.t.sizes() == want, op, a.name, a.t.sizes(), "must have shape ", want);
  contiguous(op, a);
}

inline void contiguous_numel(const char* op, Arg a, int64_t want) {
  CHK(a.t.numel() == want, op, a.name, a.t.numel(), "must have ", want,
      " elements");
  contiguous(op, a);
}

// rotary tables as the kernels index them: row n of a (>=N, 64) fp32 table
inline void rope_table(const char* op, Arg a, int64_t N) {
  CHK(a.t.dim() == 2 && a.t.size(0) >= N && a.t.size(1) == 64, op, a.name,
      a.t.sizes(), "must have shape (>=", N, ", 64)");
  contiguous(op, a);
}

// rows of a (..., C) tensor: the product of every dim but the last
inline int64_t leading_rows(const at::Tensor& t) {
  return c10::multiply_integers(t.sizes().slice(0, t.dim() - 1));
}

// ---- 3. divisibility ------------------------------------------------------

inline void multiple_of(const char* op, const char* what, int64_t v,
                        int64_t m) {
  CHK(v % m == 0, op, what, v, "must be a multiple of ", m);
}

// ---- 4. range -------------------------------------------------------------

// an extent that sizes a grid or is narrowed by a launcher: 1 <= v <= hi
inline int64_t extent(const char* op, const char* what, int64_t v,
                      int64_t hi) {
  CHK(v >= 1 && v <= hi, op, what, v, "must be in [1, ", hi, "]");
  return v;
}

inline int extent_int(const char* op, const char* what, int64_t v,
                      int64_t hi = INT_MAX) {
  return (int)extent(op, what, v, hi);
}

// ---- 5. device ------------------------------------------------------------

inline void same_gpu(const char* op, std::initializer_list<Arg> args) {
  const Arg& first = *args.begin();
  for (const Arg& a : args) {
    CHK(a.t.is_cuda(), op, a.name, a.t.device(), "must be on a GPU");
    CHK(a.t.device() == first.t.device(), op, a.name,
        a.t.device(), "must be on ", first.name, "'s device ",
        first.t.device());
  }
}

// Taken after validation and before allocation: makes the tensor's device
// current for the entry point's lifetime and carries that device's stream.
struct DeviceScope {
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard;
  hipStream_t stream;
  explicit DeviceScope(const at::Tensor& t)
      : guard(t.device()),
        stream(c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(
                   t.device().index())
                   .stream()) {}
};

// every launcher returns the hipGetLastError() taken right after its <<<>>>
// (legal under stream capture: it only reads the last error)
#define LAUNCH(op, call)                                             \
  do {                                                               \
    const hipError_t err_ = (call);                                  \
    TORCH_CHECK(err_ == hipSuccess, op, ": kernel launch failed: ",  \
                hipGetErrorString(err_));                            \
  } while (0)

}  // namespace chk
