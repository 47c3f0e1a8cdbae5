// LDS image helpers shared by attention_fwd.hip, attention_bwd.hip and
// sgu.hip: the XOR swizzles of their 128-B-row bf16 images and the types
// the ds_read_b64_tr_b16 builtin wants. Kept out of common.h because the
// probes under tools/ include that and define these names themselves.
#pragma once

#include "common.h"

// images read as ds_read_b128 MFMA fragments: byte ^= (row & 7) << 4,
// <= 2-way bank conflicts
__device__ __forceinline__ int swz(int row, int byte_in_row) {
  return (byte_in_row ^ ((row & 7) << 4));
}

// per-row 32-B XOR window, col ^= uk4(row) * 32, for images with 128-B rows
// read by ds_read_b64_tr_b16: the half-wave's 8 rows {kb..kb+3, kb+8..kb+11}
// split 4/4 by parity (row base 32*(row&1) dwords) and within a parity
// v(row) is a bijection onto 0..3, so the 8 rows cover all 64 banks ->
// zero-conflict tr reads. v*32 <= 96 B stays inside the 128-B row (uk-style
// *32 from the wgrad image would escape it).
__device__ __forceinline__ int uk4(int k) { return ((k & 2) >> 1) | ((k & 8) >> 2); }

// operand type and address space of __builtin_amdgcn_ds_read_tr16_b64_v4bf16
typedef __attribute__((__vector_size__(4 * sizeof(__bf16)))) __bf16 bf16x4t;
#define AS3 __attribute__((address_space(3)))
