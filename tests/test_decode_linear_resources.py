"""Build-time resource check of the decode linear kernels (CPU; hipcc
cross-compiles for gfx950 without a device), after
tests/test_attn_bwd_resources.py.

The kernels keep a few K-steps of weights in registers ahead of their use
and launch up to 16 waves per workgroup, four per SIMD, which leaves each
wave 128 VGPRs. A spill of the in-flight loads to scratch would be silent
and would put memory traffic back on the path the kernel exists to clear,
so the compiler's own resource-usage remark is read back here.
"""

import os

import pytest

from hip_resources import hipcc, kernel_resource_usage

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "..", "progen_amd", "ops", "hip", "decode_linear.hip")


@pytest.mark.skipif(hipcc() is None, reason="needs hipcc")
def test_decode_linear_kernels_use_no_scratch(tmp_path):
    usage = kernel_resource_usage(SRC, tmp_path)
    # vec: {bf16, fp32} x 3 acts; mfma: 3 acts x {1, 2} batch tiles
    vec = [k for k in usage if "dec_linear_vec_kernel" in k]
    mfma = [k for k in usage if "dec_linear_mfma_kernel" in k]
    assert len(vec) == 6 and len(mfma) == 6, sorted(usage)
    for k, u in usage.items():
        print(f"RESOURCE|{k}|{u}")
        assert u["ScratchSize"] == 0, (k, u)
        # a 1024-thread workgroup is four waves per SIMD
        assert u["VGPRs"] + u["AGPRs"] <= 128 and u["Occupancy"] >= 4, (k, u)
