"""Build-time resource check of the decode sampling kernel (CPU; hipcc
cross-compiles for gfx950 without a device), after
tests/test_decode_linear_resources.py.

Each thread keeps its four logits, four scores and four rank counters in
registers across the Philox rounds and the rank loop. A spill to scratch
would be silent, so the compiler's own resource-usage remark is read back
here and the table printed.
"""

import os

import pytest

from hip_resources import hipcc, kernel_resource_usage

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "..", "progen_amd", "ops", "hip", "decode_sample.hip")


@pytest.mark.skipif(hipcc() is None, reason="needs hipcc")
def test_decode_sample_kernels_use_no_scratch(tmp_path):
    usage = kernel_resource_usage(SRC, tmp_path)
    # one instantiation per storage type: bf16 and fp32
    kernels = [k for k in usage if "dec_sample_kernel" in k]
    assert len(kernels) == 2, sorted(usage)
    for k, u in usage.items():
        print(f"RESOURCE|{k}|{u}")
        assert u["ScratchSize"] == 0, (k, u)
