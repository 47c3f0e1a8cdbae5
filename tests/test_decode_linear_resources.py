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
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "..", "progen_amd", "ops", "hip", "decode_linear.hip")


def _hipcc():
    return shutil.which("hipcc") or (
        "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.mark.skipif(_hipcc() is None, reason="needs hipcc")
def test_decode_linear_kernels_use_no_scratch(tmp_path):
    r = subprocess.run(
        [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17",
         "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
         "-c", SRC, "-o", str(tmp_path / "decode_linear.o")],
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
    # vec: {bf16, fp32} x 3 acts; mfma: 3 acts x {1, 2} batch tiles
    vec = [k for k in usage if "dec_linear_vec_kernel" in k]
    mfma = [k for k in usage if "dec_linear_mfma_kernel" in k]
    assert len(vec) == 6 and len(mfma) == 6, sorted(usage)
    for k, u in usage.items():
        print(f"RESOURCE|{k}|{u}")
        assert u["ScratchSize"] == 0, (k, u)
        # a 1024-thread workgroup is four waves per SIMD
        assert u["VGPRs"] + u["AGPRs"] <= 128 and u["Occupancy"] >= 4, (k, u)
