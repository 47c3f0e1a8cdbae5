"""Build-time resource check of the attention backward kernels (CPU; hipcc
cross-compiles for gfx950 without a device).

The kernels run 8 waves per block, two per SIMD, which leaves each wave at
most 256 VGPRs; phase 1 alone takes 244 of them. The fused kernel's
epilogues are written so that nothing of theirs is held across the tile
loop — a spill to scratch there is silent and slow, so the compiler's own
resource-usage remark is read back here.
"""

import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "..", "progen_amd", "ops", "hip", "attention_bwd.hip")


def _hipcc():
    return shutil.which("hipcc") or (
        "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.mark.skipif(_hipcc() is None, reason="needs hipcc")
def test_attn_bwd_kernels_fit_two_waves_per_simd_without_scratch(tmp_path):
    r = subprocess.run(
        [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17",
         "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
         "-c", SRC, "-o", str(tmp_path / "attention_bwd.o")],
        capture_output=True, text=True, check=True)
    usage = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|"
                      r"Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split(" ")[0]] = int(m.group(2))
    main = {k: v for k, v in usage.items() if "attn_bwd_kernel" in k}
    assert len(main) == 2, sorted(usage)      # <false> and <true>
    for k, u in usage.items():
        print(f"RESOURCE|{k}|{u}")
        assert u["ScratchSize"] == 0, (k, u)
    for k, u in main.items():
        assert u["VGPRs"] + u["AGPRs"] <= 256 and u["Occupancy"] >= 2, (k, u)
