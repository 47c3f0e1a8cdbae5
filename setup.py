"""In-tree build of the progen_amd._C* HIP extensions listed in EXTENSIONS
(gfx950 only).

    PYTORCH_ROCM_ARCH=gfx950 python setup.py build_ext --inplace

The built .so files land next to the package (progen_amd/_C*.so) so the
repo snapshot carries them to the GPU box.
"""

import glob
import os

from setuptools import setup

os.environ.setdefault("PYTORCH_ROCM_ARCH", "gfx950")

from torch.utils.cpp_extension import BuildExtension, CUDAExtension  # noqa: E402

# Module name -> sources. Several modules, not one: the export list of each
# is pinned by its contract test (see EXTENSIONS in progen_amd/ops/dispatch.py,
# which lists the same names and says what adding a module takes). The bodies
# of the decode kernels are the decode_*_body.h headers, shared by the scalar
# kernels and decode_slots.hip; prefill_body.h is shared by prefill.hip and
# prefill_admit.hip; glu_bwd_body.h and ln_shift_bwd_body.h are
# shared by glu.hip / ln_shift.hip and bias_grad.hip.
EXTENSIONS = {
    "progen_amd._C": [
        "progen_amd/ops/hip/bindings.cpp",
        "progen_amd/ops/hip/ln_shift.hip",
        "progen_amd/ops/hip/glu.hip",
        "progen_amd/ops/hip/bias_grad.hip",
        "progen_amd/ops/hip/cross_entropy.hip",
        "progen_amd/ops/hip/adamw.hip",
        "progen_amd/ops/hip/rope_qkv.hip",
        "progen_amd/ops/hip/attention_fwd.hip",
        "progen_amd/ops/hip/attention_bwd.hip",
        "progen_amd/ops/hip/sgu.hip",
        "progen_amd/ops/hip/fp8_quant.hip",
        "progen_amd/ops/hip/colsum.hip",
    ],
    # the fused kernels of the cached decode step (progen_amd/decode.py)
    "progen_amd._C_decode": [
        "progen_amd/ops/hip/decode_bindings.cpp",
        "progen_amd/ops/hip/decode_ln_shift.hip",
        "progen_amd/ops/hip/decode_attn.hip",
        "progen_amd/ops/hip/decode_sgu.hip",
    ],
    # the decode step's linear op with fused epilogues
    "progen_amd._C_decode_linear": [
        "progen_amd/ops/hip/decode_linear_bindings.cpp",
        "progen_amd/ops/hip/decode_linear.hip",
    ],
    # the decode step's sampler
    "progen_amd._C_decode_sample": [
        "progen_amd/ops/hip/decode_sample_bindings.cpp",
        "progen_amd/ops/hip/decode_sample.hip",
    ],
    # the kernels that fill the decode caches from one forward over the prime
    "progen_amd._C_prefill": [
        "progen_amd/ops/hip/prefill_bindings.cpp",
        "progen_amd/ops/hip/prefill.hip",
        "progen_amd/ops/hip/prefill_admit.hip",
    ],
    # the decode kernels with one position per batch row (progen_amd/engine.py)
    "progen_amd._C_decode_slots": [
        "progen_amd/ops/hip/decode_slots_bindings.cpp",
        "progen_amd/ops/hip/decode_slots.hip",
    ],
}

# Headers the .hip sources include (the decode kernel bodies among them are
# shared by five of the files above). The ninja rule generated for .hip
# sources records no header dependencies, so BuildHip drops every .hip object
# older than the newest header before ninja decides what is up to date.
HIP_HEADERS = sorted(h for h in glob.glob("progen_amd/ops/hip/*.h")
                     if not h.endswith("_hip.h"))


class BuildHip(BuildExtension):
    def build_extension(self, ext):
        newest = max(os.path.getmtime(h) for h in HIP_HEADERS)
        pattern = os.path.join(self.build_temp, "**", "ops", "hip", "*_hip.o")
        for obj in glob.glob(pattern, recursive=True):
            if os.path.getmtime(obj) < newest:
                os.remove(obj)
        super().build_extension(ext)


COMPILE_ARGS = {
    "cxx": ["-O3", "-std=c++17"],
    "nvcc": ["-O3", "-std=c++17"],
}

setup(
    name="progen_amd_ext",
    ext_modules=[
        CUDAExtension(name=name, sources=sources,
                      extra_compile_args=COMPILE_ARGS, depends=HIP_HEADERS)
        for name, sources in EXTENSIONS.items()
    ],
    cmdclass={"build_ext": BuildHip.with_options(use_ninja=True)},
)
