"""The compiler's resource-usage remark, read back for the
tests/test_*_resources.py files (CPU; hipcc cross-compiles for gfx950
without a device).

A spill to scratch, or registers grown past an occupancy step, is silent and
slow, and no numerical test sees it; each of those files holds the table of
kernels it expects and the bounds it asserts, this one the compile and the
parse.
"""

import os
import re
import shutil
import subprocess


def hipcc():
    return shutil.which("hipcc") or (
        "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def kernel_resource_usage(src, tmp_path, extra_args=()):
    """Compile the device side of ``src`` and return {kernel: {field: int}},
    the fields being SGPRs, VGPRs, AGPRs, ScratchSize, Occupancy and LDS."""
    obj = os.path.splitext(os.path.basename(src))[0] + ".o"
    r = subprocess.run(
        [hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17",
         "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
         *extra_args, "-c", src, "-o", str(tmp_path / obj)],
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
    return usage
