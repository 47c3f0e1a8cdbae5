"""Launch contract of the decode-linear extension
(progen_amd._C_decode_linear, progen_amd/ops/hip/decode_linear_bindings.cpp)
— the scheme of tests/test_decode_ext_contract.py applied to the third
module.

Checks run dtype, shape/contiguity, divisibility, range, device LAST, so
with CPU tensors a well-formed call gets all the way to the device check
and a malformed one is stopped earlier by a message that names the op and
the argument. Nothing here touches GPU memory or launches a kernel. The
extension must be built (``dispatch.ext_decode_linear()`` raises otherwise;
no skip).
"""

import pytest

from ext_contract_helpers import F16, F32, raises_first_line, t
from progen_amd.ops import dispatch


# The well-formed call, arguments in positional order: B=2, K=64, N=32.
def good():
    return dict(x=t(2, 64), w=t(32, 64), bias=t(32), act="none")


# Every act, the optional bias absent, fp32 as the second instantiation,
# and the two ends of the row range.
GOOD_VARIANTS = [
    dict(),
    dict(act="gelu"),
    dict(act="glu"),
    dict(bias=None),
    dict(bias=None, act="glu"),
    dict(x=t(2, 64, dtype=F32), w=t(32, 64, dtype=F32), bias=t(32, dtype=F32)),
    dict(x=t(2, 64, dtype=F32), w=t(32, 64, dtype=F32), bias=None,
         act="gelu"),
    dict(x=t(1, 64)),
    dict(x=t(32, 64)),
    dict(w=t(16, 64), bias=t(16)),
]

# (arguments replaced in the well-formed call, what the message names)
BAD = [
    (dict(act="relu"), "act"),
    (dict(x=t(2, 64, dtype=F16)), "x"),
    (dict(w=t(32, 64, dtype=F32)), "w"),
    (dict(bias=t(32, dtype=F32)), "bias"),
    (dict(x=t(2, 64, dtype=F32)), "w"),
    (dict(x=t(1, 2, 64)), "x"),
    (dict(x=t(64)), "x"),
    (dict(w=t(32, 64, 1)), "w"),
    (dict(x=t(2, 128)[:, ::2]), "x"),
    (dict(w=t(32, 128)[:, ::2]), "w"),
    (dict(w=t(64, 32).t()), "w"),
    (dict(w=t(32, 128)), "w"),
    (dict(bias=t(16)), "bias"),
    (dict(bias=t(64)[::2]), "bias"),
    (dict(x=t(2, 96), w=t(32, 96)), "K"),
    (dict(w=t(24, 64), bias=t(24)), "N"),
    (dict(w=t(48, 64), bias=t(48), act="glu"), "N"),
    (dict(x=t(0, 64)), "B"),
    (dict(x=t(33, 64)), "B"),
]


def _raises(overrides):
    return raises_first_line(dispatch.ext_decode_linear(), good, "dec_linear",
                             overrides)


def test_the_export_set_is_the_one_entry_point():
    C = dispatch.ext_decode_linear()
    assert {n for n in dir(C) if not n.startswith("_")} == {"dec_linear"}
    assert dispatch.has_ext_decode_linear()


def test_the_other_modules_keep_their_export_lists():
    for mod in (dispatch.ext(), dispatch.ext_decode()):
        assert "dec_linear" not in dir(mod)


@pytest.mark.parametrize("overrides", GOOD_VARIANTS,
                         ids=[f"variant{i}" for i in range(len(GOOD_VARIANTS))])
def test_well_formed_cpu_call_reaches_the_device_check(overrides):
    msg = _raises(overrides)
    assert msg.startswith("dec_linear: "), msg
    assert "must be on a GPU, got cpu" in msg, msg


@pytest.mark.parametrize(
    "overrides,what", BAD,
    ids=[f"{what}-{i}" for i, (_, what) in enumerate(BAD)])
def test_malformed_call_is_stopped_before_the_device_check(overrides, what):
    msg = _raises(overrides)
    assert msg.startswith(f"dec_linear: {what} must "), msg
    assert ", got " in msg, msg
    assert "GPU" not in msg and "device" not in msg, msg


def test_messages_say_what_was_expected_and_what_came():
    assert _raises(dict(x=t(33, 64))) == \
        "dec_linear: B must be in [1, 32], got 33"
    assert _raises(dict(x=t(2, 96), w=t(32, 96))) == \
        "dec_linear: K must be a multiple of 64, got 96"
    assert _raises(dict(w=t(48, 64), bias=t(48), act="glu")) == \
        "dec_linear: N must be a multiple of 32, got 48"
    assert _raises(dict(act="relu")) == \
        "dec_linear: act must be one of none, gelu, glu, got relu"
