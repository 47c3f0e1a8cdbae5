"""HIP extension loading and dispatch policy.

Policy (MI355X-native, no multi-backend dispatch):
  - on a GPU (ROCm) device, ops MUST run the hand-written CDNA4 HIP
    kernels: if the in-tree extension is missing we raise rather than
    silently fall back to eager PyTorch;
  - on CPU, ops run the pure-PyTorch reference implementations
    (progen_amd/ops/reference.py) — that is the test oracle, not a
    compatibility layer.

The extension is built IN-TREE as ``progen_amd/_C*.so`` by
``python setup.py build_ext --inplace`` (driven by __graft_entry__.build),
with PYTORCH_ROCM_ARCH=gfx950, so the .so travels with the repo snapshot.
"""

from __future__ import annotations

import importlib
import os
from typing import Any, Dict

# Short key -> module name of every HIP extension. There are several modules,
# not one, because each module's export list is pinned by its contract test
# (tests/*_ext_contract.py assert that no entry point leaks into another
# module), so a new group of kernels comes as a module of its own. Adding one
# takes: a line here, a line with its sources in setup.py's EXTENSIONS, a
# bindings file under ops/hip/, an ``ext_*`` / ``has_ext_*`` pair below, and
# its contract test. __graft_entry__.build imports every module listed here.
EXTENSIONS = {
    "main": "progen_amd._C",
    "decode": "progen_amd._C_decode",
    "decode_linear": "progen_amd._C_decode_linear",
    "decode_sample": "progen_amd._C_decode_sample",
    "prefill": "progen_amd._C_prefill",
    "decode_slots": "progen_amd._C_decode_slots",
}

# key -> the imported module, or the import error as a string; an import,
# failed or not, is tried once per process
_LOADED: Dict[str, Any] = {}


def _available(key: str) -> bool:
    if key not in _LOADED:
        try:
            _LOADED[key] = importlib.import_module(EXTENSIONS[key])
        except Exception as e:  # noqa: BLE001 - record and re-raise on GPU use
            _LOADED[key] = f"{type(e).__name__}: {e}"
    return not isinstance(_LOADED[key], str)


def _load(key: str) -> Any:
    """Return the loaded extension, raising loudly if unavailable.

    Called only on the GPU path; a GPU box without the built extension is
    a deployment error, never a silent eager fallback."""
    if not _available(key):
        raise RuntimeError(
            f"progen_amd HIP extension {EXTENSIONS[key]} is not available "
            f"(import error: {_LOADED[key]}). Build it in-tree with "
            "`python setup.py build_ext --inplace` (PYTORCH_ROCM_ARCH=gfx950)."
        )
    return _LOADED[key]


def ext() -> Any:
    return _load("main")


def has_ext() -> bool:
    return _available("main")


def ext_decode() -> Any:
    return _load("decode")


def has_ext_decode() -> bool:
    return _available("decode")


def ext_decode_linear() -> Any:
    return _load("decode_linear")


def has_ext_decode_linear() -> bool:
    return _available("decode_linear")


def ext_decode_sample() -> Any:
    return _load("decode_sample")


def has_ext_decode_sample() -> bool:
    return _available("decode_sample")


def ext_prefill() -> Any:
    return _load("prefill")


def has_ext_prefill() -> bool:
    return _available("prefill")


def ext_decode_slots() -> Any:
    return _load("decode_slots")


def has_ext_decode_slots() -> bool:
    return _available("decode_slots")


def use_hip(t, op: str = None) -> bool:
    """True when tensor t lives on a ROCm GPU (→ HIP kernels are mandatory).

    Debug-only escape hatches (never the default on GPU):
    - PROGEN_FORCE_EAGER=1 routes EVERY op to its torch reference;
    - PROGEN_EAGER_OPS="attn,sgu" routes only the named ops eager —
      the per-kernel bisect lever for the graphed-replay investigation
      (profiles/r02_graphed_nan_investigation.md). Tags: ln, attn, glu,
      sgu, ce, adamw; the fused decode step's ops are dec_ln, dec_attn,
      dec_sgu, dec_linear and dec_sample (the slot step's ops answer to
      the same four); the prefill's are prefill_kv and prefill_gate.
    """
    if not t.is_cuda:
        return False
    if os.environ.get("PROGEN_FORCE_EAGER") == "1":
        return False
    if op is not None:
        eager = os.environ.get("PROGEN_EAGER_OPS")
        if eager and op in {x.strip() for x in eager.split(",")}:
            return False
    return True
