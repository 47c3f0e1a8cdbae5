"""What the tests/*_ext_contract.py files share: the tensors their tables
are written with, and the call that returns the first line of an entry
point's refusal. The GOOD / GOOD_VARIANTS / BAD tables and the tests stay in
the file of the module they describe.
"""

import pytest
import torch

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
I32, I64 = torch.int32, torch.int64


def t(*shape, dtype=BF):
    return torch.zeros(*shape, dtype=dtype)


def meta(*shape, dtype=BF):
    """Contiguous tensor of any extent with no storage behind it: reaches
    the range checks that an expanded (non-contiguous) view cannot."""
    return torch.empty(*shape, dtype=dtype, device="meta")


def raises_first_line(module, good, op, overrides):
    """Call ``module.op`` with the well-formed arguments ``good()`` (a dict
    in positional order) after replacing ``overrides`` in them; the call must
    raise RuntimeError, and the first line of its message is returned."""
    args = good()
    assert set(overrides) <= set(args), (op, overrides)
    args.update(overrides)
    with pytest.raises(RuntimeError) as ei:
        getattr(module, op)(*args.values())
    return str(ei.value).splitlines()[0]
