"""Launch contract of the prefill extension (progen_amd._C_prefill,
progen_amd/ops/hip/prefill_bindings.cpp) — the scheme of
tests/test_decode_sample_ext_contract.py applied to the fifth module.

Checks run dtype, shape/contiguity, divisibility, range, device LAST, so
with CPU tensors a well-formed call gets all the way to the device check
and a malformed one is stopped earlier by a message that names the op and
the argument. Nothing here touches GPU memory or launches a kernel. The
argument checks are skipped where the extension is not built.
"""

import pytest

from ext_contract_helpers import F16, F32, meta, raises_first_line, t
from progen_amd.ops import dispatch

needs_ext = pytest.mark.skipif(not dispatch.has_ext_prefill(),
                               reason="progen_amd._C_prefill is not built")


# The well-formed calls, arguments in positional order.
# prefill_rope_kv: B=2, Np=8, H=2, Nc=16, P=5
def good_kv():
    return dict(qkv=t(2, 8, 384), sin=t(8, 64, dtype=F32),
                cos=t(8, 64, dtype=F32), k_cache=t(2, 2, 16, 64),
                v_cache=t(2, 2, 16, 64), P=5)


# prefill_gate_ln: B=2, Np=8, d2=64, Nc=16, P=5
def good_gate():
    return dict(x=t(2, 8, 128), norm_weight=t(64), hist=t(2, 16, 64), P=5,
                eps=1e-5)


GOOD = {"prefill_rope_kv": good_kv, "prefill_gate_ln": good_gate}

GOOD_VARIANTS = [
    ("prefill_rope_kv", dict()),
    ("prefill_rope_kv", dict(P=1)),
    ("prefill_rope_kv", dict(P=8)),                       # P == Np < Nc
    ("prefill_rope_kv", dict(sin=t(20, 64, dtype=F32))),  # longer tables
    ("prefill_rope_kv", dict(k_cache=t(2, 2, 4, 64), v_cache=t(2, 2, 4, 64),
                             P=4)),                       # P == Nc < Np
    ("prefill_gate_ln", dict()),
    ("prefill_gate_ln", dict(P=1)),
    ("prefill_gate_ln", dict(P=8)),
    ("prefill_gate_ln", dict(hist=t(2, 4, 64), P=4)),
    ("prefill_gate_ln", dict(x=t(2, 8, 3072), norm_weight=t(1536),
                             hist=t(2, 16, 1536))),
]

# (op, arguments replaced in the well-formed call, what the message names)
BAD = [
    ("prefill_rope_kv", dict(qkv=t(2, 8, 384, dtype=F32)), "qkv"),
    ("prefill_rope_kv", dict(qkv=t(2, 8, 384, dtype=F16)), "qkv"),
    ("prefill_rope_kv", dict(sin=t(8, 64)), "sin"),
    ("prefill_rope_kv", dict(cos=t(8, 64, dtype=F16)), "cos"),
    ("prefill_rope_kv", dict(k_cache=t(2, 2, 16, 64, dtype=F32)), "k_cache"),
    ("prefill_rope_kv", dict(v_cache=t(2, 2, 16, 64, dtype=F32)), "v_cache"),
    ("prefill_rope_kv", dict(qkv=t(16, 384)), "qkv"),
    ("prefill_rope_kv", dict(qkv=t(2, 8, 768)[:, :, ::2]), "qkv"),
    ("prefill_rope_kv", dict(sin=t(7, 64, dtype=F32)), "sin"),
    ("prefill_rope_kv", dict(cos=t(8, 32, dtype=F32)), "cos"),
    ("prefill_rope_kv", dict(cos=t(64, 8, dtype=F32).t()), "cos"),
    ("prefill_rope_kv", dict(k_cache=t(2, 32, 64)), "k_cache"),
    ("prefill_rope_kv", dict(k_cache=t(2, 3, 16, 64)), "k_cache"),
    ("prefill_rope_kv", dict(k_cache=t(2, 2, 16, 32)), "k_cache"),
    ("prefill_rope_kv", dict(k_cache=t(2, 2, 16, 128)[..., ::2]), "k_cache"),
    ("prefill_rope_kv", dict(v_cache=t(2, 2, 8, 64)), "v_cache"),
    ("prefill_rope_kv", dict(v_cache=t(3, 2, 16, 64)), "v_cache"),
    ("prefill_rope_kv", dict(qkv=t(2, 8, 200)), "qkv.size(2)"),
    ("prefill_rope_kv", dict(qkv=t(0, 8, 384), k_cache=t(0, 2, 16, 64),
                             v_cache=t(0, 2, 16, 64)), "B"),
    ("prefill_rope_kv", dict(P=0), "P"),
    ("prefill_rope_kv", dict(P=9), "P"),     # > Np
    ("prefill_rope_kv", dict(k_cache=t(2, 2, 4, 64), v_cache=t(2, 2, 4, 64)),
     "P"),                                   # > Nc
    ("prefill_gate_ln", dict(x=t(2, 8, 128, dtype=F32)), "x"),
    ("prefill_gate_ln", dict(norm_weight=t(64, dtype=F32)), "norm_weight"),
    ("prefill_gate_ln", dict(hist=t(2, 16, 64, dtype=F32)), "hist"),
    ("prefill_gate_ln", dict(x=t(16, 128)), "x"),
    ("prefill_gate_ln", dict(x=t(2, 8, 256)[:, :, ::2]), "x"),
    ("prefill_gate_ln", dict(hist=t(32, 64)), "hist"),
    ("prefill_gate_ln", dict(x=t(2, 8, 64)), "x.size(2)"),
    ("prefill_gate_ln", dict(x=t(2, 8, 192)), "x.size(2)"),
    ("prefill_gate_ln", dict(norm_weight=t(128)), "norm_weight"),
    ("prefill_gate_ln", dict(norm_weight=t(128)[::2]), "norm_weight"),
    ("prefill_gate_ln", dict(hist=t(2, 16, 128)), "hist"),
    ("prefill_gate_ln", dict(hist=t(3, 16, 64)), "hist"),
    ("prefill_gate_ln", dict(hist=t(2, 16, 128)[..., ::2]), "hist"),
    ("prefill_gate_ln", dict(x=meta(2 ** 20, 2 ** 12, 128),
                             hist=meta(2 ** 20, 16, 64)), "B*Np"),
    ("prefill_gate_ln", dict(P=0), "P"),
    ("prefill_gate_ln", dict(P=9), "P"),
    ("prefill_gate_ln", dict(hist=t(2, 4, 64)), "P"),
]


def _raises(op, overrides):
    return raises_first_line(dispatch.ext_prefill(), GOOD[op], op, overrides)


def test_the_export_set_is_the_two_entry_points():
    C = dispatch.ext_prefill()
    assert {n for n in dir(C) if not n.startswith("_")} == \
        {"prefill_rope_kv", "prefill_gate_ln"}
    assert dispatch.has_ext_prefill()


def test_the_other_modules_keep_their_export_lists():
    for mod in (dispatch.ext(), dispatch.ext_decode(),
                dispatch.ext_decode_linear(), dispatch.ext_decode_sample()):
        assert not [n for n in dir(mod) if n.startswith("prefill")]


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
    assert _raises("prefill_rope_kv", dict(P=9)) == \
        "prefill_rope_kv: P must be in [1, 8], got 9"
    assert _raises("prefill_rope_kv", dict(v_cache=t(2, 2, 8, 64))) == \
        "prefill_rope_kv: v_cache must have shape [2, 2, 16, 64], " \
        "got [2, 2, 8, 64]"
    assert _raises("prefill_gate_ln", dict(hist=t(2, 4, 64))) == \
        "prefill_gate_ln: P must be in [1, 4], got 5"
    assert _raises("prefill_gate_ln", dict(x=t(2, 8, 192))) == \
        "prefill_gate_ln: x.size(2) must be a multiple of 128, got 192"
    assert _raises("prefill_gate_ln", dict(x=t(2, 8, 128, dtype=F32))) == \
        "prefill_gate_ln: x must have dtype BFloat16, got Float"


@needs_ext
def test_keyword_call_and_eps_default():
    C = dispatch.ext_prefill()
    args = good_gate()
    del args["eps"]
    with pytest.raises(RuntimeError, match="must be on a GPU, got cpu"):
        C.prefill_gate_ln(**args)
    with pytest.raises(RuntimeError, match="must be on a GPU, got cpu"):
        C.prefill_rope_kv(**good_kv())
