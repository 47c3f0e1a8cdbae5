"""GPU: the single-kernel attention backward (attn_bwd, fused=True).

One block walks the windows of its (batch, head) in order, hands each
window's own-band dK/dV to the next window through a thread-private fp32
carry, and writes bf16 dqkv itself. Every shape here has three windows,
so the middle one both consumes a carry and produces one (no other suite
has such a window), except the single-window shape, which has no carry at
all. Each case is held

* bit for bit to the two-kernel path (fused=False) on the same inputs, and
* to the fp64 oracle of tests/kernel_oracle.py, within the repository's
  margin times what the emulation of the kernel's bf16 storage costs on
  the same inputs (tests/KERNEL_TOLERANCES.md); nothing is a number here.

Every figure is printed as a
``KTOL|family|output|dtype|emulation|bound|measured|case`` line.
"""

import functools

import pytest
import torch

import kernel_oracle as K
from progen_amd.ops import dispatch, functional as OF, reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

CASES = [
    ("rand", 1.0, (1, 64, 1, 64)),      # one window: first and last, no carry
    ("rand", 1.0, (1, 192, 1, 64)),     # three windows, one active chunk pair
    ("rand", 1.0, (2, 384, 3, 128)),    # six blocks, two active pairs
    ("rand", 1.0, (1, 576, 1, 192)),    # three active pairs (nactive < 4)
    ("rand", 1.0, (1, 768, 2, 256)),    # the flagship window, all four pairs
    ("hot_first", 0.125, (1, 384, 2, 128)),   # dominant key in the tile that
    ("hot_last", 0.125, (1, 384, 2, 128)),    # goes through the carry
]

HALO3_SHAPE = (1, 768, 2, 128)   # joined sequence: two ranks of 3 windows


def C():
    return dispatch.ext()


def cu(t):
    return None if t is None else t.to(DEV)


def case_id(c):
    return c if isinstance(c, str) else f"{c[0]}-{c[1]}-" + "x".join(map(str, c[2]))


@functools.lru_cache(maxsize=None)
def halo3_inputs():
    """second virtual rank of a joined sequence at wsz 128, built the way
    kernel_oracle.halo_inputs builds its two-window case: three local
    windows, so dhalo at w = 0 meets carries at w = 1 and w = 2"""
    B, N, H, wsz = HALO3_SHAPE
    g = K._gen(5901)
    sin, cos = K.rope_tables(N)
    x = (K._randn(g, B, N, 3 * H * 64) * 0.5).to(K.BF16)
    dout = (K._randn(g, B, N, H * 64) * 0.5).to(K.BF16)
    L = N // 2
    tail = x[:, L - wsz:L].float().reshape(B, wsz, 3 * H, 64)[:, :, H:]
    s = sin[L - wsz:L].reshape(1, wsz, 1, 64)
    c = cos[L - wsz:L].reshape(1, wsz, 1, 64)
    halo = (tail * c + R.rotate_every_two(tail) * s).reshape(B, wsz, 2 * H * 64)
    return dict(qkv=x[:, L:].contiguous(), sin=sin[L:].contiguous(),
                cos=cos[L:].contiguous(), dout=dout[:, L:].contiguous(), H=H,
                wsz=wsz, halo=halo.to(K.BF16))


def inputs_of(case):
    return halo3_inputs() if case == "halo3" else K.attn_inputs(case)


@functools.lru_cache(maxsize=None)
def oracle_of(case):
    return K.attn_oracle(**inputs_of(case))


@functools.lru_cache(maxsize=None)
def emulation_errors(case):
    inp = inputs_of(case)
    return K.attn_errors(K.attn_emulate(inp), oracle_of(case), inp)


@functools.lru_cache(maxsize=None)
def run_both(case):
    """forward once, backward through both paths; computed once per case
    and shared by the tests, which do not change it"""
    inp = inputs_of(case)
    qkv, sin, cos, dout = (cu(inp[k]) for k in ("qkv", "sin", "cos", "dout"))
    halo = cu(inp.get("halo"))
    H, wsz = inp["H"], inp["wsz"]
    rot = C().rope_qkv(qkv, sin, cos)
    out, lse = C().attn_fwd(rot, H, wsz, halo=halo)
    res = {}
    for fused in (True, False):
        r = C().attn_bwd(dout, rot, sin, cos, out, lse, H, wsz, halo=halo,
                         fused=fused)
        got = dict(out=out, lse=lse, dqkv=r[0])
        if halo is not None:
            got["dhalo"] = r[1]
        res[fused] = got
    return res


ALL = CASES + ["halo3"]


@pytest.mark.parametrize("case", ALL, ids=case_id)
def test_fused_is_bitwise_the_two_kernel_path(case):
    got = run_both(case)
    assert torch.equal(got[True]["dqkv"], got[False]["dqkv"]), case
    if case == "halo3":
        assert torch.equal(got[True]["dhalo"], got[False]["dhalo"])


@pytest.mark.parametrize("case", ALL, ids=case_id)
def test_fused_within_margin_of_emulation(case):
    inp = inputs_of(case)
    errs = K.attn_errors(run_both(case)[True], oracle_of(case), inp)
    emu = emulation_errors(case)
    family = "attn_halo_fused" if case == "halo3" else "attn_fused"
    missed = []
    for k, v in errs.items():
        bound = K.MARGIN * emu[k]
        print(f"KTOL|{family}|{k}|bf16|{emu[k]:.3e}|{bound:.3e}|{v:.3e}|"
              f"{case_id(case)}")
        # out and lse are the forward kernels', printed for the record
        if k in ("dqkv", "dhalo") and not v <= bound:
            missed.append((k, v, bound))
    assert not missed, (case, missed)


def test_launcher_rule():
    """fused=None follows the rule that _attn_bwd_path reports; a window of
    320 needs two rounds of chunks, which only the two-kernel path has"""
    assert C()._attn_bwd_path(1, 640, 2, 320) == "two_kernel"
    assert C()._attn_bwd_path(64, 1024, 24, 256) == "fused"
    # the rule is a threshold on H*B, taken from measurement
    # (profiles/attn_bwd_fused_finalize.md): two blocks are far below it
    assert C()._attn_bwd_path(1, 768, 2, 256) == "two_kernel"

    inp = K.attn_inputs(("rand", 1.0, (1, 640, 2, 320)))
    qkv, sin, cos, dout = (cu(inp[k]) for k in ("qkv", "sin", "cos", "dout"))
    rot = C().rope_qkv(qkv, sin, cos)
    out, lse = C().attn_fwd(rot, 2, 320)
    auto = C().attn_bwd(dout, rot, sin, cos, out, lse, 2, 320)[0]
    two = C().attn_bwd(dout, rot, sin, cos, out, lse, 2, 320, fused=False)[0]
    assert torch.equal(auto, two)
    with pytest.raises(RuntimeError) as ei:
        C().attn_bwd(dout, rot, sin, cos, out, lse, 2, 320, fused=True)
    msg = str(ei.value).splitlines()[0]
    assert msg.startswith("attn_bwd: fused=True must "), msg
    assert ", got 320" in msg, msg


def test_autograd_matches_the_bindings():
    case = ("rand", 1.0, (2, 384, 3, 128))
    inp = K.attn_inputs(case)
    qkv = cu(inp["qkv"]).requires_grad_(True)
    out = OF.local_attention(qkv, cu(inp["sin"]), cu(inp["cos"]), 3, 128)
    out.backward(cu(inp["dout"]))
    got = run_both(case)[True]
    assert torch.equal(out, got["out"])
    assert torch.equal(qkv.grad, got["dqkv"])
