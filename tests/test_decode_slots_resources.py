"""Build-time resource check of the slot kernels (CPU; hipcc cross-compiles
for gfx950 without a device), after tests/test_prefill_resources.py.

The slot kernels are the bodies of the scalar decode kernels with one more
branch at the top (the idle row) and, in the sampler, five more values per
row. A spill to scratch would be silent, so the compiler's own
resource-usage remark is read back here and the table printed.
"""

import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "..", "progen_amd", "ops", "hip", "decode_slots.hip")

# kernel name -> instantiations: the LN on <BF, ONE>, the others on <BF>
EXPECTED = {"dec_ln_shift_slots_kernel": 4, "dec_attn_slots_kernel": 2,
            "dec_sgu_slots_kernel": 2, "dec_sample_slots_kernel": 2}


def _hipcc():
    return shutil.which("hipcc") or (
        "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.mark.skipif(_hipcc() is None, reason="needs hipcc")
def test_slot_kernels_use_no_scratch(tmp_path):
    r = subprocess.run(
        [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17",
         "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
         "-c", SRC, "-o", str(tmp_path / "decode_slots.o")],
        capture_output=True, text=True, check=True)
    usage = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark:\s+(SGPRs|VGPRs|AGPRs|"
                      r"ScratchSize \[bytes/lane\]|"
                      r"Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split(" ")[0]] = int(m.group(2))
    for kernel, count in EXPECTED.items():
        found = [k for k in usage if kernel in k]
        assert len(found) == count, (kernel, sorted(usage))
    # nothing but the kernels: every body is inlined into its kernel
    assert len(usage) == sum(EXPECTED.values()), sorted(usage)
    for k, u in usage.items():
        print(f"RESOURCE|{k}|{u}")
        assert u["ScratchSize"] == 0, (k, u)
