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
from typing import Any, Optional

_EXT: Optional[Any] = None
_EXT_ERR: Optional[str] = None
_TRIED = False


def _try_load() -> None:
    global _EXT, _EXT_ERR, _TRIED
    if _TRIED:
        return
    _TRIED = True
    try:
        _EXT = importlib.import_module("progen_amd._C")
    except Exception as e:  # noqa: BLE001 - record and re-raise on GPU use
        _EXT = None
        _EXT_ERR = f"{type(e).__name__}: {e}"


def ext() -> Any:
    """Return the loaded HIP extension, raising loudly if unavailable.

    Called only on the GPU path; a GPU box without the built extension is
    a deployment error, never a silent eager fallback."""
    _try_load()
    if _EXT is None:
        raise RuntimeError(
            "progen_amd HIP extension (progen_amd._C) is not available "
            f"(import error: {_EXT_ERR}). Build it in-tree with "
            "`python setup.py build_ext --inplace` (PYTORCH_ROCM_ARCH=gfx950)."
        )
    return _EXT


def has_ext() -> bool:
    _try_load()
    return _EXT is not None


# the decode-step kernels live in a second module (progen_amd._C_decode,
# ops/hip/decode_bindings.cpp); same policy, loaded on first use
_EXT_DECODE: Optional[Any] = None
_EXT_DECODE_ERR: Optional[str] = None
_TRIED_DECODE = False


def _try_load_decode() -> None:
    global _EXT_DECODE, _EXT_DECODE_ERR, _TRIED_DECODE
    if _TRIED_DECODE:
        return
    _TRIED_DECODE = True
    try:
        _EXT_DECODE = importlib.import_module("progen_amd._C_decode")
    except Exception as e:  # noqa: BLE001 - record and re-raise on GPU use
        _EXT_DECODE = None
        _EXT_DECODE_ERR = f"{type(e).__name__}: {e}"


def ext_decode() -> Any:
    """Return the loaded decode-kernel extension, raising loudly if
    unavailable — the fused decode step never falls back to torch ops."""
    _try_load_decode()
    if _EXT_DECODE is None:
        raise RuntimeError(
            "progen_amd decode extension (progen_amd._C_decode) is not "
            f"available (import error: {_EXT_DECODE_ERR}). Build it in-tree "
            "with `python setup.py build_ext --inplace` "
            "(PYTORCH_ROCM_ARCH=gfx950)."
        )
    return _EXT_DECODE


def has_ext_decode() -> bool:
    _try_load_decode()
    return _EXT_DECODE is not None


# the decode step's linear op with fused epilogues: a third module
# (progen_amd._C_decode_linear, ops/hip/decode_linear_bindings.cpp)
_EXT_DECODE_LINEAR: Optional[Any] = None
_EXT_DECODE_LINEAR_ERR: Optional[str] = None
_TRIED_DECODE_LINEAR = False


def _try_load_decode_linear() -> None:
    global _EXT_DECODE_LINEAR, _EXT_DECODE_LINEAR_ERR, _TRIED_DECODE_LINEAR
    if _TRIED_DECODE_LINEAR:
        return
    _TRIED_DECODE_LINEAR = True
    try:
        _EXT_DECODE_LINEAR = importlib.import_module(
            "progen_amd._C_decode_linear")
    except Exception as e:  # noqa: BLE001 - record and re-raise on GPU use
        _EXT_DECODE_LINEAR = None
        _EXT_DECODE_LINEAR_ERR = f"{type(e).__name__}: {e}"


def ext_decode_linear() -> Any:
    """Return the loaded decode-linear extension, raising loudly if
    unavailable — a shape routed to the kernel never falls back."""
    _try_load_decode_linear()
    if _EXT_DECODE_LINEAR is None:
        raise RuntimeError(
            "progen_amd decode-linear extension "
            "(progen_amd._C_decode_linear) is not available (import error: "
            f"{_EXT_DECODE_LINEAR_ERR}). Build it in-tree with "
            "`python setup.py build_ext --inplace` "
            "(PYTORCH_ROCM_ARCH=gfx950)."
        )
    return _EXT_DECODE_LINEAR


def has_ext_decode_linear() -> bool:
    _try_load_decode_linear()
    return _EXT_DECODE_LINEAR is not None


# the decode step's sampler: a fourth module
# (progen_amd._C_decode_sample, ops/hip/decode_sample_bindings.cpp)
_EXT_DECODE_SAMPLE: Optional[Any] = None
_EXT_DECODE_SAMPLE_ERR: Optional[str] = None
_TRIED_DECODE_SAMPLE = False


def _try_load_decode_sample() -> None:
    global _EXT_DECODE_SAMPLE, _EXT_DECODE_SAMPLE_ERR, _TRIED_DECODE_SAMPLE
    if _TRIED_DECODE_SAMPLE:
        return
    _TRIED_DECODE_SAMPLE = True
    try:
        _EXT_DECODE_SAMPLE = importlib.import_module(
            "progen_amd._C_decode_sample")
    except Exception as e:  # noqa: BLE001 - record and re-raise on GPU use
        _EXT_DECODE_SAMPLE = None
        _EXT_DECODE_SAMPLE_ERR = f"{type(e).__name__}: {e}"


def ext_decode_sample() -> Any:
    """Return the loaded decode-sample extension, raising loudly if
    unavailable — device sampling never falls back to the host sampler."""
    _try_load_decode_sample()
    if _EXT_DECODE_SAMPLE is None:
        raise RuntimeError(
            "progen_amd decode-sample extension "
            "(progen_amd._C_decode_sample) is not available (import error: "
            f"{_EXT_DECODE_SAMPLE_ERR}). Build it in-tree with "
            "`python setup.py build_ext --inplace` "
            "(PYTORCH_ROCM_ARCH=gfx950)."
        )
    return _EXT_DECODE_SAMPLE


def has_ext_decode_sample() -> bool:
    _try_load_decode_sample()
    return _EXT_DECODE_SAMPLE is not None


# the kernels that prefill the decode caches from one forward over the
# prime: a fifth module (progen_amd._C_prefill, ops/hip/prefill_bindings.cpp)
_EXT_PREFILL: Optional[Any] = None
_EXT_PREFILL_ERR: Optional[str] = None
_TRIED_PREFILL = False


def _try_load_prefill() -> None:
    global _EXT_PREFILL, _EXT_PREFILL_ERR, _TRIED_PREFILL
    if _TRIED_PREFILL:
        return
    _TRIED_PREFILL = True
    try:
        _EXT_PREFILL = importlib.import_module("progen_amd._C_prefill")
    except Exception as e:  # noqa: BLE001 - record and re-raise on GPU use
        _EXT_PREFILL = None
        _EXT_PREFILL_ERR = f"{type(e).__name__}: {e}"


def ext_prefill() -> Any:
    """Return the loaded prefill extension, raising loudly if unavailable —
    a prefill on a GPU never falls back to torch ops."""
    _try_load_prefill()
    if _EXT_PREFILL is None:
        raise RuntimeError(
            "progen_amd prefill extension (progen_amd._C_prefill) is not "
            f"available (import error: {_EXT_PREFILL_ERR}). Build it in-tree "
            "with `python setup.py build_ext --inplace` "
            "(PYTORCH_ROCM_ARCH=gfx950)."
        )
    return _EXT_PREFILL


def has_ext_prefill() -> bool:
    _try_load_prefill()
    return _EXT_PREFILL is not None


# the decode kernels with one position per batch row: a sixth module
# (progen_amd._C_decode_slots, ops/hip/decode_slots_bindings.cpp)
_EXT_DECODE_SLOTS: Optional[Any] = None
_EXT_DECODE_SLOTS_ERR: Optional[str] = None
_TRIED_DECODE_SLOTS = False


def _try_load_decode_slots() -> None:
    global _EXT_DECODE_SLOTS, _EXT_DECODE_SLOTS_ERR, _TRIED_DECODE_SLOTS
    if _TRIED_DECODE_SLOTS:
        return
    _TRIED_DECODE_SLOTS = True
    try:
        _EXT_DECODE_SLOTS = importlib.import_module(
            "progen_amd._C_decode_slots")
    except Exception as e:  # noqa: BLE001 - record and re-raise on GPU use
        _EXT_DECODE_SLOTS = None
        _EXT_DECODE_SLOTS_ERR = f"{type(e).__name__}: {e}"


def ext_decode_slots() -> Any:
    """Return the loaded slot-kernel extension, raising loudly if
    unavailable — the slot step never falls back to torch ops."""
    _try_load_decode_slots()
    if _EXT_DECODE_SLOTS is None:
        raise RuntimeError(
            "progen_amd decode-slots extension "
            "(progen_amd._C_decode_slots) is not available (import error: "
            f"{_EXT_DECODE_SLOTS_ERR}). Build it in-tree with "
            "`python setup.py build_ext --inplace` "
            "(PYTORCH_ROCM_ARCH=gfx950)."
        )
    return _EXT_DECODE_SLOTS


def has_ext_decode_slots() -> bool:
    _try_load_decode_slots()
    return _EXT_DECODE_SLOTS is not None


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
