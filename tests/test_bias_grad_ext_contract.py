"""The optional ``db`` argument of glu_bwd and ln_shift_res_bwd
(progen_amd._C) under the launch contract of tests/test_ext_contract.py: a
well-formed call with ``db`` gets as far as the device check, a malformed
``db`` is refused before it, by name. CPU tensors only; the extension must
be built (dispatch.ext() raises otherwise; no skip).
"""

import pytest
import torch

from ext_contract_helpers import F32, raises_first_line, t
from progen_amd.ops import dispatch

# entry point -> its well-formed arguments, in positional order
GOOD = {
    "glu_bwd": lambda: dict(dy=t(1, 64, 16), h=t(1, 64, 32),
                            db=t(32, dtype=F32)),
    "ln_shift_res_bwd": lambda: dict(
        dy=t(1, 64, 16), ds=t(1, 64, 16), s_in=t(1, 64, 16), g=t(16),
        mean=t(64, dtype=F32), rstd=t(64, dtype=F32), shift=True,
        db=t(16, dtype=F32)),
}

GOOD_VARIANTS = [
    ("glu_bwd", dict(db=None)),
    ("glu_bwd", dict(dy=t(1, 64, 16, dtype=F32), h=t(1, 64, 32, dtype=F32))),
    ("ln_shift_res_bwd", dict(db=None)),
    ("ln_shift_res_bwd", dict(ds=None)),
]

# (entry point, overrides, the argument the refusal must name)
BAD = [
    ("glu_bwd", dict(db=t(32)), "db"),                      # dtype
    ("glu_bwd", dict(db=t(32, dtype=torch.float64)), "db"),
    ("glu_bwd", dict(db=t(16, dtype=F32)), "db"),           # extent: H, not 2H
    ("glu_bwd", dict(db=t(1, 32, dtype=F32)), "db"),        # rank
    ("glu_bwd", dict(db=t(64, dtype=F32)[::2]), "db"),      # contiguity
    ("ln_shift_res_bwd", dict(db=t(16)), "db"),
    ("ln_shift_res_bwd", dict(db=t(32, dtype=F32)), "db"),
    ("ln_shift_res_bwd", dict(db=t(1, 16, dtype=F32)), "db"),
    ("ln_shift_res_bwd", dict(db=t(32, dtype=F32)[::2]), "db"),
    # the other arguments are still checked, and first
    ("glu_bwd", dict(dy=t(1, 64, 32)), "dy"),
    ("ln_shift_res_bwd", dict(g=t(8)), "g"),
]


def _raises(op, overrides):
    return raises_first_line(dispatch.ext(), GOOD[op], op, overrides)


@pytest.mark.parametrize(
    "op,overrides", [(op, {}) for op in GOOD] + GOOD_VARIANTS,
    ids=lambda v: v if isinstance(v, str) else ",".join(v) or "full")
def test_well_formed_cpu_call_with_db_reaches_the_device_check(op, overrides):
    msg = _raises(op, overrides)
    assert msg.startswith(f"{op}: "), msg
    assert "must be on a GPU, got cpu" in msg, msg


@pytest.mark.parametrize(
    "op,overrides,what", BAD,
    ids=[f"{op}-{what}-{i}" for i, (op, _, what) in enumerate(BAD)])
def test_malformed_db_is_stopped_before_the_device_check(op, overrides, what):
    msg = _raises(op, overrides)
    assert msg.startswith(f"{op}: {what} must "), msg
    assert "must be on a GPU" not in msg, msg


def test_db_is_a_keyword_with_default_none():
    """The positional calls of before still bind; ``db`` can be named."""
    C = dispatch.ext()
    for op in GOOD:
        args = GOOD[op]()
        db = args.pop("db")
        with pytest.raises(RuntimeError, match="must be on a GPU"):
            getattr(C, op)(*args.values())
        with pytest.raises(RuntimeError, match="must be on a GPU"):
            getattr(C, op)(*args.values(), db=db)
