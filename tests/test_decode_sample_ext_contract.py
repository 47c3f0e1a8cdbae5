"""Launch contract of the decode-sample extension
(progen_amd._C_decode_sample, progen_amd/ops/hip/decode_sample_bindings.cpp)
— the scheme of tests/test_decode_ext_contract.py applied to the fourth
module.

Checks run dtype, shape/contiguity, divisibility, range, device LAST, so
with CPU tensors a well-formed call gets all the way to the device check
and a malformed one is stopped earlier by a message that names the op and
the argument. Nothing here touches GPU memory or launches a kernel. The
extension must be built (``dispatch.ext_decode_sample()`` raises otherwise;
no skip).
"""

import pytest
import torch

from ext_contract_helpers import (F16, F32, I32, I64, meta,
                                  raises_first_line, t)
from progen_amd.ops import dispatch


def ints(*shape):
    return torch.zeros(shape, dtype=I64)


# The well-formed call, arguments in positional order: B=2, V=7, L=8.
def good():
    return dict(logits=t(2, 7), pos=ints(), seed=ints(1), seq=ints(2, 8),
                lens=ints(2), pads=ints(2), token=ints(2), top_k=3,
                greedy=False, u_out=None)


# fp32 as the second instantiation, the optional output, both ends of V and
# of top_k, greedy.
GOOD_VARIANTS = [
    dict(),
    dict(logits=t(2, 7, dtype=F32)),
    dict(u_out=t(2, 7, dtype=F32)),
    dict(greedy=True, top_k=0),
    dict(top_k=0),
    dict(top_k=7),
    dict(logits=t(2, 2), top_k=1),
    dict(logits=t(2, 1024), top_k=25),
    dict(seq=ints(2, 1)),
]

# (arguments replaced in the well-formed call, what the message names)
BAD = [
    (dict(logits=t(2, 7, dtype=F16)), "logits"),
    (dict(pos=torch.zeros((), dtype=I32)), "pos"),
    (dict(pos=torch.zeros((), dtype=F32)), "pos"),
    (dict(seed=torch.zeros(1, dtype=I32)), "seed"),
    (dict(seq=torch.zeros(2, 8, dtype=I32)), "seq"),
    (dict(lens=torch.zeros(2, dtype=I32)), "lens"),
    (dict(pads=torch.zeros(2, dtype=F32)), "pads"),
    (dict(token=torch.zeros(2, dtype=I32)), "token"),
    (dict(u_out=t(2, 7)), "u_out"),
    (dict(logits=t(1, 2, 7)), "logits"),
    (dict(logits=t(2, 14)[:, ::2]), "logits"),
    (dict(pos=ints(1)), "pos"),
    (dict(seed=ints()), "seed"),
    (dict(seed=ints(2)), "seed"),
    (dict(seq=ints(16)), "seq"),
    (dict(seq=ints(3, 8)), "seq"),
    (dict(seq=ints(2, 16)[:, ::2]), "seq"),
    (dict(lens=ints(3)), "lens"),
    (dict(lens=ints(4)[::2]), "lens"),
    (dict(pads=ints(2, 1)), "pads"),
    (dict(token=ints(1)), "token"),
    (dict(u_out=t(2, 8, dtype=F32)), "u_out"),
    (dict(u_out=t(7, 2, dtype=F32).t()), "u_out"),
    (dict(logits=t(0, 7), seq=ints(0, 8), lens=ints(0), pads=ints(0),
          token=ints(0)), "B"),
    (dict(logits=meta(70000, 7), seq=meta(70000, 8, dtype=I64),
          lens=meta(70000, dtype=I64), pads=meta(70000, dtype=I64),
          token=meta(70000, dtype=I64)), "B"),
    (dict(logits=t(2, 1), top_k=0), "V"),
    (dict(logits=t(2, 1025)), "V"),
    (dict(seq=ints(2, 0)), "L"),
    (dict(top_k=-1), "top_k"),
    (dict(top_k=8), "top_k"),
]


def _raises(overrides):
    return raises_first_line(dispatch.ext_decode_sample(), good, "dec_sample",
                             overrides)


def test_the_export_set_is_the_one_entry_point():
    C = dispatch.ext_decode_sample()
    assert {n for n in dir(C) if not n.startswith("_")} == {"dec_sample"}
    assert dispatch.has_ext_decode_sample()


def test_the_other_modules_keep_their_export_lists():
    for mod in (dispatch.ext(), dispatch.ext_decode(),
                dispatch.ext_decode_linear()):
        assert "dec_sample" not in dir(mod)


@pytest.mark.parametrize("overrides", GOOD_VARIANTS,
                         ids=[f"variant{i}" for i in range(len(GOOD_VARIANTS))])
def test_well_formed_cpu_call_reaches_the_device_check(overrides):
    msg = _raises(overrides)
    assert msg.startswith("dec_sample: "), msg
    assert "must be on a GPU, got cpu" in msg, msg


@pytest.mark.parametrize(
    "overrides,what", BAD,
    ids=[f"{what}-{i}" for i, (_, what) in enumerate(BAD)])
def test_malformed_call_is_stopped_before_the_device_check(overrides, what):
    msg = _raises(overrides)
    assert msg.startswith(f"dec_sample: {what} must "), msg
    assert ", got " in msg, msg
    assert "GPU" not in msg and "device" not in msg, msg


def test_messages_say_what_was_expected_and_what_came():
    assert _raises(dict(logits=t(2, 1025))) == \
        "dec_sample: V must be in [2, 1024], got 1025"
    assert _raises(dict(top_k=8)) == \
        "dec_sample: top_k must be in [0, 7], got 8"
    assert _raises(dict(pos=torch.zeros((), dtype=I32))) == \
        "dec_sample: pos must have dtype Long, got Int"
    assert _raises(dict(seq=ints(3, 8))) == \
        "dec_sample: seq must have shape [2, 8], got [3, 8]"
    assert _raises(dict(
        logits=meta(70000, 7), seq=meta(70000, 8, dtype=I64),
        lens=meta(70000, dtype=I64), pads=meta(70000, dtype=I64),
        token=meta(70000, dtype=I64))) == \
        "dec_sample: B must be in [1, 65535], got 70000"


def test_keyword_call_and_optional_u_out_default():
    C = dispatch.ext_decode_sample()
    args = good()
    del args["u_out"]
    with pytest.raises(RuntimeError, match="must be on a GPU, got cpu"):
        C.dec_sample(**args)
