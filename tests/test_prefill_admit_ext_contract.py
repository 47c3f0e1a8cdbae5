"""Launch contract of the prefill entry points with their trailing ``admit``
(progen_amd/ops/hip/prefill_bindings.cpp), the scheme of
tests/test_prefill_ext_contract.py: with CPU tensors a well-formed call gets
all the way to the device check, and a malformed ``admit`` or a bad cache is
stopped earlier by a message that names the op and the argument. With
``admit`` the caches may have any number S >= 1 of rows. Nothing here touches
GPU memory or launches a kernel.
"""

import pytest

from ext_contract_helpers import F32, I32, I64, meta, raises_first_line, t
from progen_amd.ops import dispatch

needs_ext = pytest.mark.skipif(not dispatch.has_ext_prefill(),
                               reason="progen_amd._C_prefill is not built")


# prefill_rope_kv: B=2, Np=8, H=2, Nc=16, S=3, P=8
def good_kv():
    return dict(qkv=t(2, 8, 384), sin=t(8, 64, dtype=F32),
                cos=t(8, 64, dtype=F32), k_cache=t(3, 2, 16, 64),
                v_cache=t(3, 2, 16, 64), P=8, admit=t(2, 2, dtype=I64))


# prefill_gate_ln: B=2, Np=8, d2=64, Nc=16, S=3, P=8
def good_gate():
    return dict(x=t(2, 8, 128), norm_weight=t(64), hist=t(3, 16, 64), P=8,
                eps=1e-5, admit=t(2, 2, dtype=I64))


GOOD = {"prefill_rope_kv": good_kv, "prefill_gate_ln": good_gate}

GOOD_VARIANTS = [
    ("prefill_rope_kv", dict()),
    ("prefill_rope_kv", dict(k_cache=t(1, 2, 16, 64),
                             v_cache=t(1, 2, 16, 64))),      # S < B
    ("prefill_rope_kv", dict(k_cache=t(2, 2, 16, 64),
                             v_cache=t(2, 2, 16, 64), P=1)),  # S == B
    ("prefill_rope_kv", dict(admit=None, k_cache=t(2, 2, 16, 64),
                             v_cache=t(2, 2, 16, 64))),      # today's call
    ("prefill_gate_ln", dict()),
    ("prefill_gate_ln", dict(hist=t(1, 16, 64))),
    ("prefill_gate_ln", dict(hist=t(7, 4, 64), P=4)),
    ("prefill_gate_ln", dict(admit=None, hist=t(2, 16, 64))),
]

# (op, arguments replaced in the well-formed call, what the message names)
BAD = [
    ("prefill_rope_kv", dict(admit=t(2, 2, dtype=I32)), "admit"),
    ("prefill_rope_kv", dict(admit=t(2, 2, dtype=F32)), "admit"),
    ("prefill_rope_kv", dict(admit=t(2, 3, dtype=I64)), "admit"),
    ("prefill_rope_kv", dict(admit=t(3, 2, dtype=I64)), "admit"),
    ("prefill_rope_kv", dict(admit=t(4, dtype=I64)), "admit"),
    ("prefill_rope_kv", dict(admit=t(2, 4, dtype=I64)[:, ::2]), "admit"),
    ("prefill_rope_kv", dict(k_cache=t(3, 2, 16, 64, dtype=F32)), "k_cache"),
    ("prefill_rope_kv", dict(k_cache=t(3, 3, 16, 64)), "k_cache"),
    ("prefill_rope_kv", dict(k_cache=t(3, 2, 16, 128)[..., ::2]), "k_cache"),
    ("prefill_rope_kv", dict(v_cache=t(2, 2, 16, 64)), "v_cache"),  # S differs
    ("prefill_rope_kv", dict(v_cache=t(3, 2, 8, 64)), "v_cache"),
    ("prefill_rope_kv", dict(k_cache=t(0, 2, 16, 64),
                             v_cache=t(0, 2, 16, 64)), "S"),
    ("prefill_rope_kv", dict(P=9), "P"),
    ("prefill_rope_kv", dict(P=0), "P"),
    # without admit the caches still take the batch's rows
    ("prefill_rope_kv", dict(admit=None), "k_cache"),
    ("prefill_gate_ln", dict(admit=t(2, 2, dtype=I32)), "admit"),
    ("prefill_gate_ln", dict(admit=t(2, 3, dtype=I64)), "admit"),
    ("prefill_gate_ln", dict(admit=t(1, 2, dtype=I64)), "admit"),
    ("prefill_gate_ln", dict(admit=t(2, 4, dtype=I64)[:, ::2]), "admit"),
    ("prefill_gate_ln", dict(hist=t(3, 16, 64, dtype=F32)), "hist"),
    ("prefill_gate_ln", dict(hist=t(3, 16, 128)), "hist"),
    ("prefill_gate_ln", dict(hist=t(48, 64)), "hist"),
    ("prefill_gate_ln", dict(hist=t(0, 16, 64)), "S"),
    ("prefill_gate_ln", dict(hist=meta(2 ** 31, 16, 64)), "S"),
    ("prefill_gate_ln", dict(hist=t(3, 4, 64)), "P"),
    ("prefill_gate_ln", dict(admit=None), "hist"),
]


def _raises(op, overrides):
    return raises_first_line(dispatch.ext_prefill(), GOOD[op], op, overrides)


def test_the_export_set_is_still_the_two_entry_points():
    C = dispatch.ext_prefill()
    assert {n for n in dir(C) if not n.startswith("_")} == \
        {"prefill_rope_kv", "prefill_gate_ln"}


@needs_ext
@pytest.mark.parametrize(
    "op,overrides", GOOD_VARIANTS,
    ids=[f"{op}-variant{i}" for i, (op, _) in enumerate(GOOD_VARIANTS)])
def test_well_formed_cpu_call_reaches_the_device_check(op, overrides):
    msg = _raises(op, overrides)
    assert msg.startswith(f"{op}: "), msg
    assert "must be on a GPU, got cpu" in msg, msg


@needs_ext
@pytest.mark.parametrize(
    "op,overrides,what", BAD,
    ids=[f"{op}-{what}-{i}" for i, (op, _, what) in enumerate(BAD)])
def test_malformed_call_is_stopped_before_the_device_check(op, overrides,
                                                           what):
    msg = _raises(op, overrides)
    assert msg.startswith(f"{op}: {what} must "), msg
    assert ", got " in msg, msg
    assert "GPU" not in msg and "device" not in msg, msg


@needs_ext
def test_messages_say_what_was_expected_and_what_came():
    assert _raises("prefill_rope_kv", dict(admit=t(2, 2, dtype=I32))) == \
        "prefill_rope_kv: admit must have dtype Long, got Int"
    assert _raises("prefill_rope_kv", dict(admit=t(2, 3, dtype=I64))) == \
        "prefill_rope_kv: admit must have shape [2, 2], got [2, 3]"
    assert _raises("prefill_gate_ln",
                   dict(admit=t(2, 4, dtype=I64)[:, ::2])) == \
        "prefill_gate_ln: admit must be contiguous, got strides [4, 2]"
    assert _raises("prefill_gate_ln", dict(hist=t(3, 16, 128))) == \
        "prefill_gate_ln: hist must have shape [3, 16, 64], got [3, 16, 128]"
    assert _raises("prefill_rope_kv", dict(admit=None)) == \
        "prefill_rope_kv: k_cache must have shape [2, 2, 16, 64], " \
        "got [3, 2, 16, 64]"


@needs_ext
def test_admit_is_a_keyword_with_default_none():
    C = dispatch.ext_prefill()
    kv = good_kv()
    with pytest.raises(RuntimeError, match="must be on a GPU, got cpu"):
        C.prefill_rope_kv(**kv)
    del kv["admit"]
    with pytest.raises(RuntimeError, match=r"k_cache must have shape \[2, "):
        C.prefill_rope_kv(**kv)
    gate = good_gate()
    del gate["eps"]
    with pytest.raises(RuntimeError, match="must be on a GPU, got cpu"):
        C.prefill_gate_ln(**gate)
