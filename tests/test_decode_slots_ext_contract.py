"""Launch contract of the slot extension (progen_amd._C_decode_slots,
progen_amd/ops/hip/decode_slots_bindings.cpp) — the scheme of
tests/test_prefill_ext_contract.py applied to the sixth module.

Checks run dtype, shape/contiguity, divisibility, range, device LAST, so
with CPU tensors a well-formed call gets all the way to the device check
and a malformed one is stopped earlier by a message that names the op and
the argument. Nothing here touches GPU memory or launches a kernel. The
argument checks are skipped where the extension is not built.
"""

import pytest

import test_decode_ext_contract as scalar
from ext_contract_helpers import (F16, F32, I32, I64, meta,
                                  raises_first_line, t)
from progen_amd.ops import dispatch

needs_ext = pytest.mark.skipif(not dispatch.has_ext_decode_slots(),
                               reason="progen_amd._C_decode_slots is not built")


# The well-formed calls, arguments in positional order.
# dec_ln_shift_slots: B=3, D=32
def good_ln():
    return dict(h=t(3, 32), res=t(3, 32), g=t(32), prev=t(3, 32),
                pos=t(3, dtype=I64), shift=True, eps=1e-5)


# dec_attn_slots: B=3, H=2, N=128, window 64
def good_attn():
    return dict(qkv=t(3, 384), rsin=t(128, 64, dtype=F32),
                rcos=t(128, 64, dtype=F32), pos=t(3, dtype=I64),
                k_cache=t(3, 2, 128, 64), v_cache=t(3, 2, 128, 64), window=64)


# dec_sgu_slots: B=3, N=16, d2=64
def good_sgu():
    return dict(h=t(3, 128), g=t(64), hist=t(3, 16, 64), w=t(16, 16),
                bias=t(16, 1), pos=t(3, dtype=I64), eps=1e-5)


# dec_sample_slots: B=3, V=256, L=32
def good_sample():
    return dict(logits=t(3, 256), pos=t(3, dtype=I64), token=t(3, dtype=I64),
                seq=t(3, 32, dtype=I64), pads=t(3, dtype=I64),
                ctl=t(3, 5, dtype=I64), u_out=None)


GOOD = {"dec_ln_shift_slots": good_ln, "dec_attn_slots": good_attn,
        "dec_sgu_slots": good_sgu, "dec_sample_slots": good_sample}

GOOD_VARIANTS = [
    ("dec_ln_shift_slots", dict()),
    ("dec_ln_shift_slots", dict(res=None)),
    ("dec_ln_shift_slots", dict(prev=None, shift=False)),
    ("dec_ln_shift_slots", dict(h=t(3, 32, dtype=F32), res=None,
                                g=t(32, dtype=F32),
                                prev=t(3, 32, dtype=F32))),
    ("dec_ln_shift_slots", dict(h=t(3, 4096), res=t(3, 4096), g=t(4096),
                                prev=t(3, 4096))),
    ("dec_attn_slots", dict()),
    ("dec_attn_slots", dict(rsin=t(200, 64, dtype=F32))),   # longer tables
    ("dec_attn_slots", dict(qkv=t(3, 384, dtype=F32),
                            k_cache=t(3, 2, 128, 64, dtype=F32),
                            v_cache=t(3, 2, 128, 64, dtype=F32))),
    ("dec_sgu_slots", dict()),
    ("dec_sgu_slots", dict(h=t(3, 640), g=t(320), hist=t(3, 16, 320))),
    ("dec_sample_slots", dict()),
    ("dec_sample_slots", dict(u_out=t(3, 256, dtype=F32))),
    ("dec_sample_slots", dict(logits=t(3, 256, dtype=F32))),
    ("dec_sample_slots", dict(logits=t(3, 2))),
    ("dec_sample_slots", dict(logits=t(3, 1024))),
]

# (op, arguments replaced in the well-formed call, what the message names)
BAD = [
    ("dec_ln_shift_slots", dict(h=t(3, 32, dtype=F16)), "h"),
    ("dec_ln_shift_slots", dict(g=t(32, dtype=F32)), "g"),
    ("dec_ln_shift_slots", dict(pos=t(3, dtype=I32)), "pos"),
    ("dec_ln_shift_slots", dict(pos=t((), dtype=I64)), "pos"),     # 0-dim
    ("dec_ln_shift_slots", dict(pos=t(4, dtype=I64)), "pos"),
    ("dec_ln_shift_slots", dict(pos=t(6, dtype=I64)[::2]), "pos"),
    ("dec_ln_shift_slots", dict(res=t(3, 16)), "res"),
    ("dec_ln_shift_slots", dict(prev=None), "prev"),               # shift set
    ("dec_ln_shift_slots", dict(h=t(3, 24), res=None, g=t(24),
                                prev=t(3, 24)), "D"),
    ("dec_attn_slots", dict(qkv=t(3, 384, dtype=F16)), "qkv"),
    ("dec_attn_slots", dict(rsin=t(128, 64)), "rsin"),
    ("dec_attn_slots", dict(pos=t(3, dtype=F32)), "pos"),
    ("dec_attn_slots", dict(pos=t((), dtype=I64)), "pos"),         # 0-dim
    ("dec_attn_slots", dict(pos=t(2, dtype=I64)), "pos"),
    ("dec_attn_slots", dict(pos=t(3, 1, dtype=I64)), "pos"),
    ("dec_attn_slots", dict(k_cache=t(3, 2, 128, 32)), "k_cache"),
    ("dec_attn_slots", dict(v_cache=t(3, 2, 64, 64)), "v_cache"),
    ("dec_attn_slots", dict(qkv=t(3, 192)), "qkv"),
    ("dec_attn_slots", dict(rcos=t(100, 64, dtype=F32)), "rcos"),
    ("dec_attn_slots", dict(window=32), "window"),
    ("dec_attn_slots", dict(window=0), "window"),
    ("dec_attn_slots", dict(k_cache=t(3, 2, 192, 64), v_cache=t(3, 2, 192, 64),
                            rsin=t(192, 64, dtype=F32),
                            rcos=t(192, 64, dtype=F32), window=128), "N"),
    ("dec_sgu_slots", dict(h=t(3, 128, dtype=F32)), "g"),
    ("dec_sgu_slots", dict(pos=t(3, dtype=I32)), "pos"),
    ("dec_sgu_slots", dict(pos=t((), dtype=I64)), "pos"),          # 0-dim
    ("dec_sgu_slots", dict(pos=t(1, dtype=I64)), "pos"),
    ("dec_sgu_slots", dict(h=t(3, 64)), "h"),
    ("dec_sgu_slots", dict(w=t(16, 8)), "w"),
    ("dec_sgu_slots", dict(bias=t(16)), "bias"),
    ("dec_sgu_slots", dict(h=t(3, 64), g=t(32), hist=t(3, 16, 32)), "d2"),
    ("dec_sample_slots", dict(logits=t(3, 256, dtype=F16)), "logits"),
    ("dec_sample_slots", dict(pos=t(3, dtype=I32)), "pos"),
    ("dec_sample_slots", dict(pos=t((), dtype=I64)), "pos"),       # 0-dim
    ("dec_sample_slots", dict(pos=t(4, dtype=I64)), "pos"),
    ("dec_sample_slots", dict(token=t(3, dtype=I32)), "token"),
    ("dec_sample_slots", dict(token=t(2, dtype=I64)), "token"),
    ("dec_sample_slots", dict(seq=t(2, 32, dtype=I64)), "seq"),
    ("dec_sample_slots", dict(seq=t(96, dtype=I64)), "seq"),
    ("dec_sample_slots", dict(pads=t(3, 1, dtype=I64)), "pads"),
    ("dec_sample_slots", dict(ctl=t(3, 5, dtype=I32)), "ctl"),     # dtype
    ("dec_sample_slots", dict(ctl=t(3, 4, dtype=I64)), "ctl"),     # shape
    ("dec_sample_slots", dict(ctl=t(5, 3, dtype=I64)), "ctl"),
    ("dec_sample_slots", dict(ctl=t(15, dtype=I64)), "ctl"),
    ("dec_sample_slots", dict(ctl=t(3, 10, dtype=I64)[:, ::2]), "ctl"),
    ("dec_sample_slots", dict(u_out=t(3, 256)), "u_out"),
    ("dec_sample_slots", dict(u_out=t(3, 128, dtype=F32)), "u_out"),
    ("dec_sample_slots", dict(logits=t(3, 1)), "V"),
    ("dec_sample_slots", dict(logits=t(3, 1025)), "V"),
    ("dec_sample_slots", dict(logits=meta(70000, 256),
                              pos=meta(70000, dtype=I64),
                              token=meta(70000, dtype=I64),
                              seq=meta(70000, 32, dtype=I64),
                              pads=meta(70000, dtype=I64),
                              ctl=meta(70000, 5, dtype=I64)), "B"),
]


def _raises(op, overrides):
    return raises_first_line(dispatch.ext_decode_slots(), GOOD[op], op,
                             overrides)


def test_the_export_set_is_the_four_entry_points():
    C = dispatch.ext_decode_slots()
    assert {n for n in dir(C) if not n.startswith("_")} == \
        {"dec_ln_shift_slots", "dec_attn_slots", "dec_sgu_slots",
         "dec_sample_slots"}
    assert dispatch.has_ext_decode_slots()


def test_the_other_modules_keep_their_export_lists():
    for mod in (dispatch.ext(), dispatch.ext_decode(),
                dispatch.ext_decode_linear(), dispatch.ext_decode_sample(),
                dispatch.ext_prefill()):
        assert not [n for n in dir(mod) if n.endswith("_slots")]


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
    assert _raises("dec_attn_slots", dict(pos=t((), dtype=I64))) == \
        "dec_attn_slots: pos must have shape [3], got []"
    assert _raises("dec_sgu_slots", dict(pos=t(1, dtype=I64))) == \
        "dec_sgu_slots: pos must have shape [3], got [1]"
    assert _raises("dec_sample_slots", dict(ctl=t(3, 4, dtype=I64))) == \
        "dec_sample_slots: ctl must have shape [3, 5], got [3, 4]"
    assert _raises("dec_sample_slots", dict(ctl=t(3, 5, dtype=I32))) == \
        "dec_sample_slots: ctl must have dtype Long, got Int"
    assert _raises("dec_sample_slots", dict(logits=t(3, 1025))) == \
        "dec_sample_slots: V must be in [2, 1024], got 1025"


@needs_ext
def test_the_scalar_entry_points_still_refuse_a_1d_pos():
    """The slot kernels are new entry points; the old ones keep their 0-dim
    position."""
    a = good_attn()
    a.pop("window")
    with pytest.raises(RuntimeError, match="dec_attn: pos must have 0 dims"):
        dispatch.ext_decode().dec_attn(*a.values(), 64)


# The scalar step's contract, held against the slot step's. The cases are
# those of tests/test_decode_ext_contract.py for the three kernels the two
# steps share, plus each well-formed call; the slot op is called at the SCALAR
# table's shapes, so that the two messages can be compared whole. Left out:
# the cases whose override replaces ``pos``, the one argument whose rule
# differs (0 dims there, (B,) here; the tables above have those).
SCALAR_ROWS = {"dec_ln_shift": "h", "dec_attn": "k_cache", "dec_sgu": "hist"}
PARITY = [(op, {}) for op in SCALAR_ROWS] + \
    [(op, ov) for op, ov, _ in scalar.BAD if "pos" not in ov]


def _slot_args_at_scalar_shapes(op, overrides):
    """The scalar op's well-formed call with ``overrides``, as the slot op
    takes it: its own argument order, and a (B,) ``pos`` for whatever B the
    call has."""
    args = scalar.GOOD[op]()
    args.update(overrides)
    args["pos"] = t(args[SCALAR_ROWS[op]].size(0), dtype=I64)
    names = list(GOOD[op + "_slots"]())
    assert set(names) == set(args), (names, sorted(args))
    return {k: args[k] for k in names}


def test_parity_cases_cover_each_shared_kernel():
    for op in SCALAR_ROWS:
        assert sum(1 for o, ov in PARITY if o == op and ov) >= 3, op


@needs_ext
@pytest.mark.parametrize(
    "op,overrides", PARITY,
    ids=[f"{op}-{','.join(ov) or 'full'}-{i}"
         for i, (op, ov) in enumerate(PARITY)])
def test_slot_entry_refuses_what_the_scalar_entry_refuses(op, overrides):
    """Same arguments, same first complaint: the slot op's message is the
    scalar op's with the op name substituted."""
    want = scalar._raises(op, overrides)
    assert want.startswith(f"{op}: "), want
    got = raises_first_line(
        dispatch.ext_decode_slots(),
        lambda: _slot_args_at_scalar_shapes(op, overrides), op + "_slots", {})
    assert got == f"{op}_slots: " + want[len(op) + 2:], (got, want)


@needs_ext
def test_keyword_call_and_defaults():
    C = dispatch.ext_decode_slots()
    args = good_sample()
    del args["u_out"]
    with pytest.raises(RuntimeError, match="must be on a GPU, got cpu"):
        C.dec_sample_slots(**args)
    args = good_sgu()
    del args["eps"]
    with pytest.raises(RuntimeError, match="must be on a GPU, got cpu"):
        C.dec_sgu_slots(**args)
