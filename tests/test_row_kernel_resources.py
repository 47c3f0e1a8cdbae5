"""Build-time resource check of the row kernels — ln_shift, glu/gelu,
cross entropy, AdamW (CPU; hipcc cross-compiles for gfx950 without a
device), after tests/test_attn_bwd_resources.py.

These kernels are memory-bound and hide their latency behind resident
waves: a spill to scratch, or registers grown past an occupancy step, is
silent and slow, and no numerical test sees it. So the compiler's own
resource-usage remark is read back here. Every kernel runs at the full 8
waves per SIMD, except ln_shift_bwd, which keeps a row's operands in
registers across its two block sums and is held, per instantiation, to
the occupancy it had with one text per path (with one row body for both
paths it compiles to 7 or 8 everywhere; the floors are what it must
never fall below).
"""

import os
import re

import pytest

from hip_resources import hipcc, kernel_resource_usage

HERE = os.path.dirname(os.path.abspath(__file__))
HIP = os.path.join(HERE, "..", "progen_amd", "ops", "hip")

# kernels each file must define (the template instantiations counted)
KERNELS = {
    "ln_shift": {"ln_shift_fwd_kernel": 8, "ln_shift_bwd_kernel": 8},
    "glu": {"glu_fwd_kernel": 2, "glu_bwd_kernel": 2, "gelu_fwd_kernel": 2,
            "gelu_bwd_kernel": 2},
    "cross_entropy": {"ce_fwd_kernel": 2, "ce_bwd_kernel": 2},
    "adamw": {"fused_adamw_kernel": 2, "grad_sumsq_kernel": 2,
              "step_inc_kernel": 1},
}

# ln_shift_bwd_kernel<BF, SHIFT, DS>: least waves per SIMD
LN_BWD_FLOOR = {
    (1, 1, 1): 5, (1, 1, 0): 4, (1, 0, 1): 6, (1, 0, 0): 6,
    (0, 1, 1): 5, (0, 1, 0): 6, (0, 0, 1): 6, (0, 0, 0): 8,
}


@pytest.mark.skipif(hipcc() is None, reason="needs hipcc")
@pytest.mark.parametrize("name", sorted(KERNELS))
def test_row_kernels_keep_their_occupancy_without_scratch(name, tmp_path):
    usage = kernel_resource_usage(os.path.join(HIP, name + ".hip"), tmp_path)
    for kernel, count in KERNELS[name].items():
        assert sum(kernel in k for k in usage) == count, (kernel, sorted(usage))
    assert len(usage) == sum(KERNELS[name].values()), sorted(usage)
    for k, u in usage.items():
        print(f"RESOURCE|{k}|{u}")
        assert u["ScratchSize"] == 0, (k, u)
        floor = 8
        if "ln_shift_bwd_kernel" in k:
            m = re.search(r"ln_shift_bwd_kernelILb([01])ELb([01])ELb([01])E", k)
            assert m, k
            floor = LN_BWD_FLOOR[tuple(int(b) for b in m.groups())]
        assert u["Occupancy"] >= floor, (k, u, floor)
