"""Build-time resource check of the admit prefill kernels (CPU; hipcc
cross-compiles for gfx950 without a device), after
tests/test_prefill_resources.py: prefill_admit.hip holds exactly the two
kernels, neither spills to scratch, and the compiler's table is printed.
"""

import os

import pytest

from hip_resources import hipcc, kernel_resource_usage

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "..", "progen_amd", "ops", "hip", "prefill_admit.hip")


@pytest.mark.skipif(hipcc() is None, reason="needs hipcc")
def test_admit_kernels_use_no_scratch(tmp_path):
    usage = kernel_resource_usage(SRC, tmp_path)
    for kernel in ("admit_rope_kv_kernel", "admit_gate_ln_kernel"):
        assert len([k for k in usage if kernel in k]) == 1, sorted(usage)
    assert len(usage) == 2, sorted(usage)
    for k, u in usage.items():
        print(f"RESOURCE|{k}|{u}")
        assert u["ScratchSize"] == 0, (k, u)
