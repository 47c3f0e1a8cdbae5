"""Launch contract of the HIP extension (progen_amd/ops/hip/bindings.cpp).

Every kernel entry point validates its arguments in one fixed order —
dtype, shape/contiguity, divisibility, range, device LAST — before it
allocates or launches anything. Device being last is what makes this file
possible: with CPU tensors a well-formed call must get all the way to the
device check, and a malformed one must be stopped by an earlier check
whose message names the op and the offending argument.

Nothing here touches GPU memory or launches a kernel. The extension must
be built (``dispatch.ext()`` raises otherwise; no skip).
"""

import pytest
import torch

from ext_contract_helpers import (BF, F16, F32, I32, I64, meta,
                                  raises_first_line, t)
from progen_amd.ops import dispatch


def huge(*shape, dtype=BF):
    """Over-range CPU tensor without the memory: a zero-stride view."""
    return torch.zeros(1, dtype=dtype).expand(*shape)


# One well-formed call per exported kernel entry point, arguments in
# positional order. Tiny shapes: B=1, N=64, D=16; attention H=1, wsz=64;
# sgu N=256, D=64; adamw one 16-element chunk.
GOOD = {
    "ln_shift_fwd": lambda: dict(x=t(1, 64, 16), g=t(16), shift=True, eps=1e-5),
    "ln_shift_res_fwd": lambda: dict(
        x=t(1, 64, 16), res=t(1, 64, 16), g=t(16), shift=True, eps=1e-5),
    "ln_shift_bwd": lambda: dict(
        dy=t(1, 64, 16), x=t(1, 64, 16), g=t(16), mean=t(64, dtype=F32),
        rstd=t(64, dtype=F32), shift=True),
    "ln_shift_res_bwd": lambda: dict(
        dy=t(1, 64, 16), ds=t(1, 64, 16), s_in=t(1, 64, 16), g=t(16),
        mean=t(64, dtype=F32), rstd=t(64, dtype=F32), shift=True),
    "glu_fwd": lambda: dict(h=t(1, 64, 32)),
    "glu_bwd": lambda: dict(dy=t(1, 64, 16), h=t(1, 64, 32)),
    "gelu_fwd": lambda: dict(h=t(1, 64, 16)),
    "gelu_bwd": lambda: dict(dy=t(1, 64, 16), h=t(1, 64, 16)),
    "ce_fwd": lambda: dict(logits=t(1, 64, 16), targets=t(1, 64, dtype=I64)),
    "ce_bwd": lambda: dict(
        dnll=t(1, 64, dtype=F32), logits=t(1, 64, 16),
        targets=t(1, 64, dtype=I64), lse=t(1, 64, dtype=F32)),
    "grad_sumsq": lambda: dict(grads=t(16)),
    "fused_adamw": lambda: dict(
        master=t(16, dtype=F32), params=t(16), grads=t(16),
        exp_avg=t(16, dtype=F32), exp_avg_sq=t(16, dtype=F32),
        chunk_starts=torch.tensor([0], dtype=I64),
        chunk_ends=torch.tensor([16], dtype=I64),
        chunk_decay=torch.tensor([1], dtype=I32),
        lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2,
        step_dev=t(1, dtype=I32), grad_scale=1.0,
        clip_coef=torch.ones(1), shard_off=0),
    "rope_qkv": lambda: dict(
        qkv=t(1, 64, 192), rsin=t(64, 64, dtype=F32), rcos=t(64, 64, dtype=F32)),
    "attn_fwd": lambda: dict(
        qkv_rot=t(1, 64, 192), heads=1, window=64, halo=t(1, 64, 128)),
    "attn_bwd": lambda: dict(
        dout=t(1, 64, 64), qkv=t(1, 64, 192), rsin=t(64, 64, dtype=F32),
        rcos=t(64, 64, dtype=F32), out=t(1, 64, 64),
        lse=t(1, 1, 64, dtype=F32), heads=1, window=64, halo=t(1, 64, 128)),
    "sgu_fwd": lambda: dict(
        xa=t(1, 256, 64), g_ln=t(1, 256, 64), w=t(256, 256),
        bias=t(256, 1, dtype=F32)),
    "sgu_dgate": lambda: dict(t_in=t(1, 256, 64), w=t(256, 256)),
    "sgu_dw": lambda: dict(
        t_in=t(1, 256, 64), g_ln=t(1, 256, 64), tri_m=t(10, dtype=I32),
        tri_k=t(10, dtype=I32)),
    "colsum": lambda: dict(dy=t(64, 16)),
    "fp8_quantize": lambda: dict(t=t(16), scale=torch.ones(1)),
    "fp8_quantize_t": lambda: dict(w=t(2, 16), scale=torch.ones(1)),
}

# Optional tensors may also be absent.
GOOD_VARIANTS = [
    ("ln_shift_res_bwd", dict(ds=None)),
    ("attn_fwd", dict(halo=None)),
    ("attn_bwd", dict(halo=None)),
]

def _attn_bwd_meta(B):
    return dict(dout=meta(B, 64, 64), qkv=meta(B, 64, 192),
                out=meta(B, 64, 64), lse=meta(B, 1, 64, dtype=F32),
                halo=meta(B, 64, 128))


# (op, arguments replaced in the well-formed call, what the message must
# name). Grouped per op by rule class: dtype, shape/length, contiguity,
# divisibility, range. ``huge`` cases are stopped by the contiguity rule
# (a zero-stride view is not contiguous); ``meta`` cases reach the range
# rule itself.
BAD = [
    # ---- ln_shift: g reinterpreted with x's vector type ----
    ("ln_shift_fwd", dict(g=t(16, dtype=F32)), "g"),
    ("ln_shift_fwd", dict(g=t(8)), "g"),
    ("ln_shift_fwd", dict(x=t(1, 64, 16, dtype=F16), g=t(16, dtype=F16)), "x"),
    ("ln_shift_fwd", dict(x=t(64, 16)), "x"),
    ("ln_shift_fwd", dict(x=t(1, 64, 32)[..., ::2]), "x"),
    ("ln_shift_fwd", dict(x=t(1, 64, 24), g=t(24)), "D"),
    ("ln_shift_fwd", dict(x=huge(1 << 20, 1 << 12, 16)), "x"),
    ("ln_shift_fwd", dict(x=meta(1 << 20, 1 << 12, 16)), "B*N"),
    ("ln_shift_res_fwd", dict(g=t(16, dtype=F32)), "g"),
    ("ln_shift_res_fwd", dict(g=t(32)), "g"),
    ("ln_shift_res_fwd", dict(res=t(1, 64, 16, dtype=F32)), "res"),
    ("ln_shift_res_fwd", dict(res=t(1, 32, 16)), "res"),
    ("ln_shift_res_fwd", dict(res=t(1, 64, 32)[..., ::2]), "res"),
    ("ln_shift_res_fwd",
     dict(x=t(1, 64, 24), res=t(1, 64, 24), g=t(24)), "D"),
    ("ln_shift_res_fwd",
     dict(x=meta(1 << 20, 1 << 12, 16), res=meta(1 << 20, 1 << 12, 16)), "B*N"),
    ("ln_shift_bwd", dict(g=t(16, dtype=F32)), "g"),
    ("ln_shift_bwd", dict(g=t(8)), "g"),
    ("ln_shift_bwd", dict(mean=t(63, dtype=F32)), "mean"),
    ("ln_shift_bwd", dict(mean=t(64)), "mean"),
    ("ln_shift_bwd", dict(rstd=t(1, dtype=F32)), "rstd"),
    ("ln_shift_bwd", dict(dy=t(1, 64, 16, dtype=F32)), "dy"),
    ("ln_shift_bwd", dict(dy=t(1, 64, 8)), "dy"),
    ("ln_shift_bwd", dict(dy=t(1, 64, 32)[..., ::2]), "dy"),
    ("ln_shift_bwd", dict(dy=t(1, 64, 24), x=t(1, 64, 24), g=t(24)), "D"),
    ("ln_shift_bwd",
     dict(dy=meta(1 << 20, 1 << 12, 16), x=meta(1 << 20, 1 << 12, 16),
          mean=meta(1 << 32, dtype=F32), rstd=meta(1 << 32, dtype=F32)), "B*N"),
    ("ln_shift_res_bwd", dict(g=t(16, dtype=F32)), "g"),
    ("ln_shift_res_bwd", dict(g=t(8)), "g"),
    ("ln_shift_res_bwd", dict(mean=t(32, dtype=F32)), "mean"),
    ("ln_shift_res_bwd", dict(ds=t(1, 64, 16, dtype=F32)), "ds"),
    ("ln_shift_res_bwd", dict(ds=t(1, 64, 8)), "ds"),
    ("ln_shift_res_bwd", dict(s_in=t(1, 64, 32)[..., ::2]), "s_in"),
    ("ln_shift_res_bwd",
     dict(dy=t(1, 64, 24), ds=None, s_in=t(1, 64, 24), g=t(24)), "D"),
    # ---- glu / gelu ----
    ("glu_fwd", dict(h=t(1, 64, 32, dtype=F16)), "h"),
    ("glu_fwd", dict(h=t(1, 64, 64)[..., ::2]), "h"),
    ("glu_fwd", dict(h=t(1, 64, 24)), "H2"),
    ("glu_fwd", dict(h=t(0, 32)), "rows"),
    ("glu_fwd", dict(h=meta(1, 1 << 32)), "H2"),
    ("glu_bwd", dict(dy=t(1, 64, 16, dtype=F32)), "dy"),
    ("glu_bwd", dict(dy=t(1, 64, 32)), "dy"),
    ("glu_bwd", dict(dy=t(1, 64, 32)[..., ::2]), "dy"),
    ("glu_bwd", dict(dy=t(1, 64, 12), h=t(1, 64, 24)), "H2"),
    ("gelu_fwd", dict(h=t(1, 64, 16, dtype=I32)), "h"),
    ("gelu_fwd", dict(h=t(1, 64, 32)[..., ::2]), "h"),
    ("gelu_fwd", dict(h=t(12)), "h.numel()"),
    ("gelu_fwd", dict(h=t(0)), "h.numel()"),
    ("gelu_bwd", dict(dy=t(1, 64, 16, dtype=F32)), "dy"),
    ("gelu_bwd", dict(dy=t(1, 32, 16)), "dy"),
    ("gelu_bwd", dict(dy=t(1, 64, 32)[..., ::2]), "dy"),
    ("gelu_bwd", dict(dy=t(12), h=t(12)), "h.numel()"),
    # ---- cross entropy: one target per logits row ----
    ("ce_fwd", dict(targets=t(1, 63, dtype=I64)), "targets"),
    ("ce_fwd", dict(targets=t(1, 64, dtype=I32)), "targets"),
    ("ce_fwd", dict(logits=t(1, 64, 16, dtype=F16)), "logits"),
    ("ce_fwd", dict(logits=t(1, 64, 32)[..., ::2]), "logits"),
    ("ce_fwd", dict(targets=t(1, 128, dtype=I64)[:, ::2]), "targets"),
    ("ce_fwd", dict(logits=huge(1 << 34, 4)), "logits"),
    ("ce_fwd",
     dict(logits=meta(1 << 34, 4), targets=meta(1 << 34, dtype=I64)), "rows"),
    ("ce_fwd",
     dict(logits=meta(1, 1 << 31), targets=meta(1, dtype=I64)), "V"),
    ("ce_bwd", dict(targets=t(1, 63, dtype=I64)), "targets"),
    ("ce_bwd", dict(targets=t(1, 64, dtype=I32)), "targets"),
    ("ce_bwd", dict(dnll=t(1, 64)), "dnll"),
    ("ce_bwd", dict(dnll=t(1, 32, dtype=F32)), "dnll"),
    ("ce_bwd", dict(lse=t(1, 32, dtype=F32)), "lse"),
    ("ce_bwd", dict(lse=t(1, 128, dtype=F32)[:, ::2]), "lse"),
    # ---- fused adamw ----
    ("grad_sumsq", dict(grads=t(16, dtype=F16)), "grads"),
    ("grad_sumsq", dict(grads=t(32)[::2]), "grads"),
    ("grad_sumsq", dict(grads=t(12)), "grads.numel()"),
    ("grad_sumsq", dict(grads=t(0)), "grads.numel()"),
    ("fused_adamw", dict(params=t(16, dtype=F16), grads=t(16, dtype=F16)),
     "params"),
    ("fused_adamw", dict(grads=t(16, dtype=F32)), "grads"),
    ("fused_adamw", dict(grads=t(8)), "grads"),
    ("fused_adamw", dict(master=t(16)), "master"),
    ("fused_adamw", dict(master=t(32, dtype=F32)[::2]), "master"),
    ("fused_adamw", dict(exp_avg=t(8, dtype=F32)), "exp_avg"),
    ("fused_adamw", dict(exp_avg_sq=t(8, dtype=F32)), "exp_avg_sq"),
    ("fused_adamw", dict(shard_off=-1), "shard_off"),
    ("fused_adamw", dict(shard_off=1), "shard_off + master.numel()"),
    ("fused_adamw", dict(chunk_ends=t(2, dtype=I64)), "chunk_ends"),
    ("fused_adamw", dict(chunk_decay=t(2, dtype=I32)), "chunk_decay"),
    ("fused_adamw", dict(chunk_starts=t(1, dtype=I32)), "chunk_starts"),
    ("fused_adamw", dict(chunk_decay=t(1, dtype=I64)), "chunk_decay"),
    ("fused_adamw", dict(step_dev=t(1, dtype=I64)), "step_dev"),
    ("fused_adamw", dict(step_dev=t(2, dtype=I32)), "step_dev"),
    ("fused_adamw", dict(clip_coef=t(1)), "clip_coef"),
    ("fused_adamw", dict(clip_coef=torch.ones(2)), "clip_coef"),
    ("fused_adamw",
     dict(chunk_starts=t(0, dtype=I64), chunk_ends=t(0, dtype=I64),
          chunk_decay=t(0, dtype=I32)), "nchunks"),
    # ---- attention ----
    ("rope_qkv", dict(qkv=t(1, 64, 192, dtype=F32)), "qkv"),
    ("rope_qkv", dict(rsin=t(64, 64)), "rsin"),
    ("rope_qkv", dict(rsin=t(32, 64, dtype=F32)), "rsin"),
    ("rope_qkv", dict(rcos=t(64, 32, dtype=F32)), "rcos"),
    ("rope_qkv", dict(rcos=t(64, 128, dtype=F32)[:, ::2]), "rcos"),
    ("rope_qkv", dict(qkv=t(1, 64, 128)), "qkv.size(2)"),
    ("rope_qkv", dict(qkv=t(0, 64, 192)), "B"),
    ("attn_fwd", dict(qkv_rot=t(1, 64, 192, dtype=F32)), "qkv_rot"),
    ("attn_fwd", dict(halo=t(1, 64, 128, dtype=F32)), "halo"),
    ("attn_fwd", dict(halo=t(1, 32, 128)), "halo"),
    ("attn_fwd", dict(halo=t(1, 64, 64)), "halo"),
    ("attn_fwd", dict(halo=t(1, 64, 256)[..., ::2]), "halo"),
    ("attn_fwd", dict(qkv_rot=t(1, 64, 384)), "qkv_rot.size(2)"),
    ("attn_fwd", dict(window=32, qkv_rot=t(1, 64, 192), halo=None), "window"),
    ("attn_fwd", dict(qkv_rot=t(1, 96, 192)), "N"),
    ("attn_fwd", dict(heads=70000), "heads"),
    ("attn_fwd", dict(heads=0), "heads"),
    ("attn_fwd", dict(qkv_rot=huge(70000, 64, 192)), "qkv_rot"),
    ("attn_fwd",
     dict(qkv_rot=meta(70000, 64, 192), halo=meta(70000, 64, 128)), "B"),
    ("attn_bwd", dict(lse=t(1, 64, dtype=F32)), "lse"),
    ("attn_bwd", dict(lse=t(1, 1, 64)), "lse"),
    ("attn_bwd", dict(out=t(1, 64, 128)), "out"),
    ("attn_bwd", dict(out=t(1, 64, 64, dtype=F32)), "out"),
    ("attn_bwd", dict(dout=t(1, 64, 64, dtype=F32)), "dout"),
    ("attn_bwd", dict(dout=t(1, 64, 128)[..., ::2]), "dout"),
    ("attn_bwd", dict(rsin=t(64, 32, dtype=F32)), "rsin"),
    ("attn_bwd", dict(rsin=t(32, 64, dtype=F32)), "rsin"),
    ("attn_bwd", dict(rcos=t(64, 64)), "rcos"),
    ("attn_bwd", dict(halo=t(1, 32, 128)), "halo"),
    ("attn_bwd", dict(qkv=t(1, 64, 384)), "qkv.size(2)"),
    ("attn_bwd", dict(window=32, halo=None), "window"),
    ("attn_bwd", dict(heads=70000), "heads"),
    ("attn_bwd", _attn_bwd_meta(70000), "B"),
    # ---- sgu ----
    ("sgu_fwd", dict(g_ln=t(1, 256, 64, dtype=F32)), "g_ln"),
    ("sgu_fwd", dict(xa=t(1, 256, 64, dtype=F32)), "xa"),
    ("sgu_fwd", dict(g_ln=t(1, 256, 32)), "g_ln"),
    ("sgu_fwd", dict(w=t(256, 128)), "w"),
    ("sgu_fwd", dict(w=t(256, 512)[:, ::2]), "w"),
    ("sgu_fwd", dict(bias=t(128, dtype=F32)), "bias"),
    ("sgu_fwd", dict(xa=t(1, 128, 64), g_ln=t(1, 128, 64), w=t(128, 128),
                     bias=t(128, dtype=F32)), "N"),
    ("sgu_fwd", dict(xa=t(1, 256, 32), g_ln=t(1, 256, 32)), "D"),
    ("sgu_fwd", dict(xa=meta(70000, 256, 64), g_ln=meta(70000, 256, 64)), "B"),
    ("sgu_dgate", dict(w=t(256, 128)), "w"),
    ("sgu_dgate", dict(w=t(256, 256, dtype=F32)), "w"),
    ("sgu_dgate", dict(t_in=t(1, 256, 128)[..., ::2]), "t_in"),
    ("sgu_dgate", dict(t_in=t(1, 128, 64), w=t(128, 128)), "N"),
    ("sgu_dgate", dict(t_in=t(1, 256, 32)), "D"),
    ("sgu_dgate", dict(t_in=huge(70000, 256, 64)), "t_in"),
    ("sgu_dgate", dict(t_in=meta(70000, 256, 64)), "B"),
    ("sgu_dw", dict(tri_k=t(9, dtype=I32)), "tri_k"),
    ("sgu_dw", dict(tri_m=t(10, dtype=I64)), "tri_m"),
    ("sgu_dw", dict(g_ln=t(1, 256, 32)), "g_ln"),
    ("sgu_dw", dict(g_ln=t(1, 256, 64, dtype=F32)), "g_ln"),
    ("sgu_dw", dict(tri_m=t(20, dtype=I32)[::2]), "tri_m"),
    ("sgu_dw", dict(t_in=t(1, 96, 64), g_ln=t(1, 96, 64)), "N"),
    ("sgu_dw", dict(t_in=t(1, 256, 48), g_ln=t(1, 256, 48)), "D"),
    ("sgu_dw", dict(tri_m=t(0, dtype=I32), tri_k=t(0, dtype=I32)),
     "tri_m.numel()"),
    ("sgu_dw", dict(t_in=meta(70000, 256, 64), g_ln=meta(70000, 256, 64)), "B"),
    # ---- colsum / fp8 ----
    ("colsum", dict(dy=t(64, 16, dtype=F32)), "dy"),
    ("colsum", dict(dy=t(64)), "dy"),
    ("colsum", dict(dy=t(64, 32)[:, ::2]), "dy"),
    ("colsum", dict(dy=t(64, 12)), "C"),
    ("colsum", dict(dy=t(0, 16)), "R"),
    ("colsum", dict(dy=meta(1 << 32, 8)), "R"),
    ("fp8_quantize", dict(t=t(16, dtype=F32)), "t"),
    ("fp8_quantize", dict(scale=t(1)), "scale"),
    ("fp8_quantize", dict(scale=torch.ones(2)), "scale"),
    ("fp8_quantize", dict(t=t(32)[::2]), "t"),
    ("fp8_quantize", dict(t=t(12)), "t.numel()"),
    ("fp8_quantize_t", dict(w=t(2, 16, dtype=F32)), "w"),
    ("fp8_quantize_t", dict(w=t(32)), "w"),
    ("fp8_quantize_t", dict(w=t(2, 32)[:, ::2]), "w"),
    ("fp8_quantize_t", dict(scale=torch.ones(2)), "scale"),
    ("fp8_quantize_t", dict(w=t(3, 16)), "rows"),
    ("fp8_quantize_t", dict(w=meta(1 << 32, 2)), "rows"),
]


def _raises(op, overrides):
    return raises_first_line(dispatch.ext(), GOOD[op], op, overrides)


def test_every_kernel_entry_point_is_covered():
    """GOOD lists every exported name except the host-only crc32c."""
    C = dispatch.ext()
    exported = {n for n in dir(C) if not n.startswith("_")}
    assert exported - {"crc32c"} == set(GOOD)
    for op in GOOD:
        assert sum(1 for b in BAD if b[0] == op) >= 3, op


@pytest.mark.parametrize(
    "op,overrides", [(op, {}) for op in GOOD] + GOOD_VARIANTS,
    ids=lambda v: v if isinstance(v, str) else ",".join(v) or "full")
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


def test_range_checks_report_the_extent():
    """The range rule itself (not contiguity) stops an over-range extent,
    and says what it got."""
    assert _raises("attn_fwd", dict(
        qkv_rot=meta(70000, 64, 192), halo=None)) == \
        "attn_fwd: B must be in [1, 65535], got 70000"
    assert _raises("ln_shift_fwd", dict(x=meta(1 << 20, 1 << 12, 16))) == \
        f"ln_shift_fwd: B*N must be in [1, {2**31 - 1}], got {1 << 32}"


def test_crc32c_unchanged():
    assert dispatch.ext().crc32c(b"123456789") == 0xE3069283
