"""Build-time resource check of the slot kernels (CPU; hipcc cross-compiles
for gfx950 without a device), after tests/test_prefill_resources.py.

The slot kernels are the bodies of the scalar decode kernels with one more
branch at the top (the idle row) and, in the sampler, five more values per
row. A spill to scratch would be silent, so the compiler's own
resource-usage remark is read back here and the table printed.
"""

import os

import pytest

from hip_resources import hipcc, kernel_resource_usage

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "..", "progen_amd", "ops", "hip", "decode_slots.hip")

# kernel name -> instantiations: the LN on <BF, ONE>, the others on <BF>
EXPECTED = {"dec_ln_shift_slots_kernel": 4, "dec_attn_slots_kernel": 2,
            "dec_sgu_slots_kernel": 2, "dec_sample_slots_kernel": 2}


@pytest.mark.skipif(hipcc() is None, reason="needs hipcc")
def test_slot_kernels_use_no_scratch(tmp_path):
    usage = kernel_resource_usage(SRC, tmp_path)
    for kernel, count in EXPECTED.items():
        found = [k for k in usage if kernel in k]
        assert len(found) == count, (kernel, sorted(usage))
    # nothing but the kernels: every body is inlined into its kernel
    assert len(usage) == sum(EXPECTED.values()), sorted(usage)
    for k, u in usage.items():
        print(f"RESOURCE|{k}|{u}")
        assert u["ScratchSize"] == 0, (k, u)
