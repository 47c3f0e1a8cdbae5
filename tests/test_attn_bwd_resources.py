"""Build-time resource check of the attention backward kernels (CPU; hipcc
cross-compiles for gfx950 without a device).

The kernels run 8 waves per block, two per SIMD, which leaves each wave at
most 256 VGPRs; phase 1 alone takes 244 of them. The fused kernel's
epilogues are written so that nothing of theirs is held across the tile
loop — a spill to scratch there is silent and slow, so the compiler's own
resource-usage remark is read back here.
"""

import os

import pytest

from hip_resources import hipcc, kernel_resource_usage

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "..", "progen_amd", "ops", "hip", "attention_bwd.hip")


@pytest.mark.skipif(hipcc() is None, reason="needs hipcc")
def test_attn_bwd_kernels_fit_two_waves_per_simd_without_scratch(tmp_path):
    usage = kernel_resource_usage(SRC, tmp_path)
    main = {k: v for k, v in usage.items() if "attn_bwd_kernel" in k}
    assert len(main) == 2, sorted(usage)      # <false> and <true>
    for k, u in usage.items():
        print(f"RESOURCE|{k}|{u}")
        assert u["ScratchSize"] == 0, (k, u)
    for k, u in main.items():
        assert u["VGPRs"] + u["AGPRs"] <= 256 and u["Occupancy"] >= 2, (k, u)
