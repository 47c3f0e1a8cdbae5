"""Build-time resource check of the bias-gradient kernels (bias_grad.hip),
after tests/test_row_kernel_resources.py (CPU; hipcc cross-compiles for
gfx950 without a device).

glu_bwd_db_kernel and ln_shift_bwd_db_kernel are glu_bwd_kernel and
ln_shift_bwd_kernel plus a per-column sum of what they store. They are as
memory-bound as those two, so a spill to scratch or a lost occupancy step is
as silent and as slow. The floors are the occupancies of the build whose
speed profiles/fused_bias_grad.md records: 8 waves per SIMD for every
instantiation (the column sums cost no occupancy step: glu_bwd_db compiles to
49 (bf16) / 60 (fp32) VGPRs, ln_shift_bwd_db to 58..64).
"""

import os

import pytest

from hip_resources import hipcc, kernel_resource_usage

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "..", "progen_amd", "ops", "hip", "bias_grad.hip")

# kernels the file must define (the template instantiations counted), and
# the least waves per SIMD of each
KERNELS = {"glu_bwd_db_kernel": 2, "ln_shift_bwd_db_kernel": 8}
FLOOR = 8


@pytest.mark.skipif(hipcc() is None, reason="needs hipcc")
def test_bias_grad_kernels_keep_their_occupancy_without_scratch(tmp_path):
    usage = kernel_resource_usage(SRC, tmp_path)
    for kernel, count in KERNELS.items():
        assert sum(kernel in k for k in usage) == count, (kernel, sorted(usage))
    assert len(usage) == sum(KERNELS.values()), sorted(usage)
    for k, u in usage.items():
        print(f"RESOURCE|{k}|{u}")
        assert u["ScratchSize"] == 0, (k, u)
        assert u["Occupancy"] >= FLOOR, (k, u, FLOOR)
