"""Launch contract of the decode extension (progen_amd._C_decode,
progen_amd/ops/hip/decode_bindings.cpp) — the scheme of
tests/test_ext_contract.py applied to the second module.

Checks run dtype, shape/contiguity, divisibility, range, device LAST, so
with CPU tensors a well-formed call gets all the way to the device check
and a malformed one is stopped earlier by a message that names the op and
the argument. Nothing here touches GPU memory or launches a kernel. The
extension must be built (``dispatch.ext_decode()`` raises otherwise; no
skip).
"""

import pytest
import torch

from ext_contract_helpers import (F16, F32, I32, I64, meta,
                                  raises_first_line, t)
from progen_amd.ops import dispatch


def pos(dtype=I64):
    return torch.zeros((), dtype=dtype)


# One well-formed call per entry point, arguments in positional order.
# Tiny shapes: B=1, D=16; attention H=1, N=64, window=64; sgu N=64, d2=64.
GOOD = {
    "dec_ln_shift": lambda: dict(
        h=t(1, 16), res=t(1, 16), g=t(16), prev=t(1, 16), shift=True,
        eps=1e-5),
    "dec_attn": lambda: dict(
        qkv=t(1, 192), rsin=t(64, 64, dtype=F32), rcos=t(64, 64, dtype=F32),
        pos=pos(), k_cache=t(1, 1, 64, 64), v_cache=t(1, 1, 64, 64),
        window=64),
    "dec_sgu": lambda: dict(
        h=t(1, 128), g=t(64), hist=t(1, 64, 64), w=t(64, 64), bias=t(64, 1),
        pos=pos(), eps=1e-5),
}

# Optional tensors may also be absent; fp32 is the second instantiation.
GOOD_VARIANTS = [
    ("dec_ln_shift", dict(res=None)),
    ("dec_ln_shift", dict(prev=None, shift=False)),
    ("dec_ln_shift", dict(h=t(1, 16, dtype=F32), res=t(1, 16, dtype=F32),
                          g=t(16, dtype=F32), prev=t(1, 16, dtype=F32))),
    ("dec_attn", dict(rsin=t(128, 64, dtype=F32))),
    ("dec_attn", dict(qkv=t(1, 192, dtype=F32),
                      k_cache=t(1, 1, 64, 64, dtype=F32),
                      v_cache=t(1, 1, 64, 64, dtype=F32))),
    ("dec_sgu", dict(h=t(1, 128, dtype=F32), g=t(64, dtype=F32),
                     hist=t(1, 64, 64, dtype=F32), w=t(64, 64, dtype=F32),
                     bias=t(64, 1, dtype=F32))),
]

# (op, arguments replaced in the well-formed call, what the message names)
BAD = [
    # ---- dec_ln_shift ----
    ("dec_ln_shift", dict(h=t(1, 16, dtype=F16)), "h"),
    ("dec_ln_shift", dict(res=t(1, 16, dtype=F32)), "res"),
    ("dec_ln_shift", dict(g=t(16, dtype=F32)), "g"),
    ("dec_ln_shift", dict(prev=t(1, 16, dtype=F32)), "prev"),
    ("dec_ln_shift", dict(h=t(1, 1, 16)), "h"),
    ("dec_ln_shift", dict(h=t(1, 32)[:, ::2]), "h"),
    ("dec_ln_shift", dict(res=t(2, 16)), "res"),
    ("dec_ln_shift", dict(g=t(8)), "g"),
    ("dec_ln_shift", dict(prev=t(1, 32)[:, ::2]), "prev"),
    ("dec_ln_shift", dict(prev=None), "prev"),
    ("dec_ln_shift",
     dict(h=t(1, 24), res=t(1, 24), g=t(24), prev=t(1, 24)), "D"),
    ("dec_ln_shift",
     dict(h=meta(70000, 16), res=meta(70000, 16), prev=meta(70000, 16)), "B"),
    ("dec_ln_shift", dict(h=t(0, 16), res=t(0, 16), prev=t(0, 16)), "B"),
    # ---- dec_attn ----
    ("dec_attn", dict(window=0), "window"),
    ("dec_attn", dict(qkv=t(1, 192, dtype=F16)), "qkv"),
    ("dec_attn", dict(rsin=t(64, 64)), "rsin"),
    ("dec_attn", dict(rcos=t(64, 64)), "rcos"),
    ("dec_attn", dict(pos=pos(F32)), "pos"),
    ("dec_attn", dict(pos=pos(I32)), "pos"),
    ("dec_attn", dict(k_cache=t(1, 1, 64, 64, dtype=F32)), "k_cache"),
    ("dec_attn", dict(v_cache=t(1, 1, 64, 64, dtype=F32)), "v_cache"),
    ("dec_attn", dict(k_cache=t(1, 64, 64)), "k_cache"),
    ("dec_attn", dict(k_cache=t(1, 1, 64, 32), v_cache=t(1, 1, 64, 32)),
     "k_cache"),
    ("dec_attn", dict(k_cache=t(1, 1, 64, 128)[..., ::2]), "k_cache"),
    ("dec_attn", dict(v_cache=t(1, 1, 128, 64)), "v_cache"),
    ("dec_attn", dict(qkv=t(1, 128)), "qkv"),
    ("dec_attn", dict(qkv=t(2, 192)), "qkv"),
    ("dec_attn", dict(rsin=t(32, 64, dtype=F32)), "rsin"),
    ("dec_attn", dict(rcos=t(64, 32, dtype=F32)), "rcos"),
    ("dec_attn", dict(pos=t(1, dtype=I64)), "pos"),
    ("dec_attn", dict(window=96), "window"),
    ("dec_attn", dict(window=128), "N"),
    ("dec_attn",
     dict(qkv=meta(70000, 192), k_cache=meta(70000, 1, 64, 64),
          v_cache=meta(70000, 1, 64, 64)), "B*H"),
    # ---- dec_sgu ----
    ("dec_sgu", dict(h=t(1, 128, dtype=F16)), "h"),
    ("dec_sgu", dict(g=t(64, dtype=F32)), "g"),
    ("dec_sgu", dict(hist=t(1, 64, 64, dtype=F32)), "hist"),
    ("dec_sgu", dict(w=t(64, 64, dtype=F32)), "w"),
    ("dec_sgu", dict(bias=t(64, 1, dtype=F32)), "bias"),
    ("dec_sgu", dict(pos=pos(F32)), "pos"),
    ("dec_sgu", dict(hist=t(64, 64)), "hist"),
    ("dec_sgu", dict(hist=t(1, 64, 128)[..., ::2]), "hist"),
    ("dec_sgu", dict(h=t(1, 64)), "h"),
    ("dec_sgu", dict(g=t(32)), "g"),
    ("dec_sgu", dict(w=t(64, 32)), "w"),
    ("dec_sgu", dict(w=t(64, 128)[:, ::2]), "w"),
    ("dec_sgu", dict(bias=t(64)), "bias"),
    ("dec_sgu", dict(pos=t(1, dtype=I64)), "pos"),
    ("dec_sgu", dict(h=t(1, 64), g=t(32), hist=t(1, 64, 32)), "d2"),
    ("dec_sgu", dict(h=meta(70000, 128), hist=meta(70000, 64, 64)), "B"),
]


def _raises(op, overrides):
    return raises_first_line(dispatch.ext_decode(), GOOD[op], op, overrides)


def test_every_decode_entry_point_is_covered():
    C = dispatch.ext_decode()
    exported = {n for n in dir(C) if not n.startswith("_")}
    assert exported == set(GOOD)
    for op in GOOD:
        assert sum(1 for b in BAD if b[0] == op) >= 3, op


def test_decode_extension_leaves_the_main_export_list_alone():
    """The decode entry points live in their own module: none leaked into
    progen_amd._C (whose exact export list tests/test_ext_contract.py
    pins), and has_ext_decode() reports the built module."""
    assert dispatch.has_ext_decode()
    main = {n for n in dir(dispatch.ext()) if not n.startswith("_")}
    assert not main & set(GOOD)


@pytest.mark.parametrize(
    "op,overrides", [(op, {}) for op in GOOD] + GOOD_VARIANTS,
    ids=[op for op in GOOD] +
        [f"{op}-variant{i}" for i, (op, _) in enumerate(GOOD_VARIANTS)])
def test_well_formed_cpu_call_reaches_the_device_check(op, overrides):
    msg = _raises(op, overrides)
    assert msg.startswith(f"{op}: "), msg
    assert "must be on a GPU, got cpu" in msg, msg


@pytest.mark.parametrize(
    "op,overrides,what", BAD,
    ids=[f"{op}-{what}-{i}" for i, (op, _, what) in enumerate(BAD)])
def test_malformed_call_is_stopped_before_the_device_check(op, overrides, what):
    msg = _raises(op, overrides)
    assert msg.startswith(f"{op}: {what} must "), msg
    assert ", got " in msg, msg
    assert "GPU" not in msg and "device" not in msg, msg


def test_messages_say_what_was_expected_and_what_came():
    assert _raises("dec_attn", dict(window=96)) == \
        "dec_attn: window must be a multiple of 64, got 96"
    assert _raises("dec_ln_shift", dict(
        h=t(1, 24), res=t(1, 24), g=t(24), prev=t(1, 24))) == \
        "dec_ln_shift: D must be a multiple of 16, got 24"
    assert _raises("dec_attn", dict(pos=pos(F32))) == \
        "dec_attn: pos must have dtype Long, got Float"
    assert _raises("dec_ln_shift", dict(prev=None)) == \
        "dec_ln_shift: prev must be given when shift is set, got None"
    assert _raises("dec_sgu", dict(
        h=meta(70000, 128), hist=meta(70000, 64, 64))) == \
        "dec_sgu: B must be in [1, 65535], got 70000"
