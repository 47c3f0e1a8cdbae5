"""Build-time resource check of the prefill kernels (CPU; hipcc
cross-compiles for gfx950 without a device), after
tests/test_decode_sample_resources.py.

Both are row kernels that hold a row's 16 B vectors in registers between
their passes. A spill to scratch would be silent, so the compiler's own
resource-usage remark is read back here and the table printed.
"""

import os

import pytest

from hip_resources import hipcc, kernel_resource_usage

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "..", "progen_amd", "ops", "hip", "prefill.hip")


@pytest.mark.skipif(hipcc() is None, reason="needs hipcc")
def test_prefill_kernels_use_no_scratch(tmp_path):
    usage = kernel_resource_usage(SRC, tmp_path)
    for kernel in ("prefill_rope_kv_kernel", "prefill_gate_ln_kernel"):
        assert len([k for k in usage if kernel in k]) == 1, sorted(usage)
    assert len(usage) == 2, sorted(usage)
    for k, u in usage.items():
        print(f"RESOURCE|{k}|{u}")
        assert u["ScratchSize"] == 0, (k, u)
