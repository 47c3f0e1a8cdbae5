"""Differentiable ProGen ops with CPU-reference / HIP-kernel dispatch.

GPU path: hand-written CDNA4 HIP kernels (progen_amd/ops/hip/) via the
in-tree extension ``progen_amd._C`` — mandatory on GPU (no silent eager
fallback; see ops/dispatch.py). Plain GEMMs (QKV/FF/out projections, the
SGU spatial matmul) go through torch.matmul = hipBLASLt, which is the
library-GEMM path, not a compatibility layer.

CPU path: the pure-PyTorch fp32 reference (ops/reference.py), which is
also the numerics oracle for the kernels.
"""

from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import dispatch, reference


# ---------------------------------------------------------------------------
# bias gradients taken from the consumer's backward kernel
# ---------------------------------------------------------------------------
# The output gradient of a biased linear is summed over its rows for the bias
# gradient; torch's linear_backward does that with a separate reduce that
# re-reads the tensor the NEXT backward kernel has just stored. Where that
# kernel is one of ours (glu_bwd for proj_in, ln_shift_res_bwd for to_out and
# ff.proj_out) it sums what it stores on the way out (ops/hip/bias_grad.hip).
# The two halves belong together: the linear is called with a detached bias,
# so it computes no bias gradient, IF AND ONLY IF its consumer op is handed
# the bias parameter and delivers the gradient. ``fused_dbias`` is the one
# predicate that decides both, evaluated once per call site.

def fused_dbias(x: torch.Tensor, weight: torch.Tensor, bias, tag: str) -> bool:
    """True when the linear ``(weight, bias)`` applied to ``x`` leaves its
    bias gradient to its consumer op ``tag`` ("glu" or "ln"): the consumer
    runs its HIP kernel, the linear is torch's own, and
    ``PROGEN_FUSED_DBIAS`` (read at call time) is not 0."""
    if bias is None or not bias.requires_grad:
        return False
    if os.environ.get("PROGEN_FUSED_DBIAS", "1") == "0":
        return False
    if not dispatch.use_hip(x, tag):  # CPU, PROGEN_FORCE_EAGER, PROGEN_EAGER_OPS
        return False
    from . import fp8, overlap
    if fp8.fp8_eligible(x, weight):
        return False
    # the custom linear Function computes its own dbias
    return not (overlap.ENABLED or overlap.FN_LINEAR)


def _bias_grad_buffer(bias_dtype, n: int, device):
    """The fp32 ``db`` a backward kernel fills, or None without a bias."""
    if bias_dtype is None:
        return None
    return torch.empty(n, dtype=torch.float32, device=device)


# ---------------------------------------------------------------------------
# fused LayerNorm(scale-only) + token shift
# ---------------------------------------------------------------------------

class _LnShiftFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, shift: bool, eps: float):
        C = dispatch.ext()
        y, mean, rstd = C.ln_shift_fwd(x, weight, bool(shift), float(eps))
        ctx.save_for_backward(x, weight, mean, rstd)
        ctx.shift = bool(shift)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, mean, rstd = ctx.saved_tensors
        C = dispatch.ext()
        dx, dweight = C.ln_shift_bwd(dy.contiguous(), x, weight, mean, rstd, ctx.shift)
        return dx, dweight, None, None


def ln_shift(x: torch.Tensor, weight: torch.Tensor, shift: bool = True,
             eps: float = 1e-5) -> torch.Tensor:
    """LN (scale-only, reference: progen.py:22) + optional token shift
    (reference: progen.py:43-46), fused on GPU."""
    if dispatch.use_hip(x, "ln"):
        return _LnShiftFn.apply(x, weight, shift, eps)
    return reference.ln_shift(x, weight, shift, eps)


class _LnShiftResFn(torch.autograd.Function):
    """Residual-add-fused LN+shift: forms s = x + res in-kernel (bf16
    rounding identical to an eager add), normalizes s, and returns
    (y, s) — s is the new residual stream. Backward returns the SAME
    gradient tensor for x and res (d(x+res) fans out identically); both
    are intermediate activations here, never leaves, so sharing is safe
    and saves the autograd accumulation pass.

    ``res_bias`` (optional) is the bias of the linear that produced ``res``,
    unused in forward: dx is that linear's output gradient, so the backward
    kernel also sums it per column and the sum is returned as the bias's
    gradient (see ``fused_dbias``)."""

    @staticmethod
    def forward(ctx, x, res, weight, shift: bool, eps: float, res_bias=None):
        C = dispatch.ext()
        y, s, mean, rstd = C.ln_shift_res_fwd(x, res, weight, bool(shift),
                                              float(eps))
        ctx.save_for_backward(s, weight, mean, rstd)
        ctx.shift = bool(shift)
        ctx.bias_dtype = None if res_bias is None else res_bias.dtype
        ctx.set_materialize_grads(False)
        return y, s

    @staticmethod
    def backward(ctx, dy, ds):
        s, weight, mean, rstd = ctx.saved_tensors
        C = dispatch.ext()
        ds = ds.contiguous() if ds is not None else None
        db = _bias_grad_buffer(ctx.bias_dtype, s.shape[-1], s.device)
        dx, dweight = C.ln_shift_res_bwd(dy.contiguous(), ds, s, weight,
                                         mean, rstd, ctx.shift, db)
        if db is not None:
            db = db.to(ctx.bias_dtype)
        return dx, dx, dweight, None, None, db


def ln_shift_res(x: torch.Tensor, res, weight: torch.Tensor,
                 shift: bool = True, eps: float = 1e-5, res_bias=None):
    """Residual add + LN + shift in one pass: returns (y, s) with
    s = x + res (the updated residual stream) and y = ln_shift(s).
    ``res=None`` degenerates to plain ln_shift with s = x.

    ``res_bias``: the bias parameter of the linear that produced ``res``,
    given exactly when ``fused_dbias`` said so for that linear (which then ran
    with the bias detached); its gradient comes out of this op's backward."""
    hip = dispatch.use_hip(x, "ln")
    if res_bias is not None and (res is None or not hip):
        raise RuntimeError("ln_shift_res: res_bias needs the HIP kernel and a "
                           "res to deliver its gradient (see fused_dbias)")
    if hip:
        if res is None:
            return _LnShiftFn.apply(x, weight, shift, eps), x
        return _LnShiftResFn.apply(x, res.contiguous(), weight, shift, eps,
                                   res_bias)
    s = x if res is None else x + res
    return reference.ln_shift(s, weight, shift, eps), s


# ---------------------------------------------------------------------------
# fused local window attention (rotary + window + softmax + AV)
# ---------------------------------------------------------------------------

class _LocalAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, sin, cos, heads: int, window_size: int, halo):
        C = dispatch.ext()
        # pre-rotation pass (rotary on q, k AND v — progen.py:87); the
        # attention kernels then stage pure bf16 copies
        qkv_rot = C.rope_qkv(qkv.contiguous(), sin, cos)
        out, lse = C.attn_fwd(qkv_rot, int(heads), int(window_size),
                              halo=halo)
        ctx.save_for_backward(qkv_rot, sin, cos, out, lse,
                              *([halo] if halo is not None else []))
        ctx.heads = int(heads)
        ctx.window_size = int(window_size)
        ctx.has_halo = halo is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv_rot, sin, cos, out, lse = ctx.saved_tensors[:5]
        halo = ctx.saved_tensors[5] if ctx.has_halo else None
        C = dispatch.ext()
        # bwd finalize applies the inverse rotation (rotary is linear)
        res = C.attn_bwd(dout.contiguous(), qkv_rot, sin, cos, out, lse,
                         ctx.heads, ctx.window_size, halo=halo)
        dqkv = res[0]
        # the halo holds PRE-ROTATED [k|v]: its grad stays in rotated
        # space (the peer applies the inverse rotation after receiving
        # it, with its own absolute positions — parallel/cp.py)
        dhalo = res[1].to(dout.dtype) if ctx.has_halo else None
        return dqkv, None, None, None, None, dhalo


def local_attention(qkv: torch.Tensor, sin: torch.Tensor, cos: torch.Tensor,
                    heads: int, window_size: int,
                    halo: torch.Tensor = None) -> torch.Tensor:
    """Fused windowed-causal attention core (reference: progen.py:83-103).

    Applies interleaved rotary to q, k AND v (quirk, progen.py:87), windows
    the sequence with one-window lookback (window 0's zero lookback keys
    UNMASKED, progen.py:90-96), runs online-softmax attention on MFMA and
    returns the merged (B, N, h*dh) context.

    ``halo``: optional (B, wsz, 2*H*dh) ROTATED [k|v] band that replaces
    window 0's zero lookback (context parallelism, parallel/cp.py); its
    gradient (same shape/space) is returned to the autograd graph."""
    if dispatch.use_hip(qkv, "attn"):
        return _LocalAttnFn.apply(qkv, sin, cos, heads, window_size, halo)
    assert halo is None, "halo is a kernel-path (GPU) feature"
    return reference.local_attention(qkv, sin, cos, heads, window_size)


# ---------------------------------------------------------------------------
# GLU-GELU epilogue
# ---------------------------------------------------------------------------

class _GluGeluFn(torch.autograd.Function):
    """``bias`` (optional) is the bias of the linear that produced ``h``,
    unused in forward: dh is that linear's output gradient, so the backward
    kernel also sums it per column and the sum is returned as the bias's
    gradient (see ``fused_dbias``)."""

    @staticmethod
    def forward(ctx, h, bias=None):
        C = dispatch.ext()
        y = C.glu_fwd(h)
        ctx.save_for_backward(h)
        ctx.bias_dtype = None if bias is None else bias.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        (h,) = ctx.saved_tensors
        C = dispatch.ext()
        db = _bias_grad_buffer(ctx.bias_dtype, h.shape[-1], h.device)
        dh = C.glu_bwd(dy.contiguous(), h, db)
        if db is not None:
            db = db.to(ctx.bias_dtype)
        return dh, db


def glu_gelu(h: torch.Tensor, bias=None) -> torch.Tensor:
    """x, gate = split(h, 2); x * gelu(gate)  (reference: progen.py:139-141).

    ``bias``: the bias parameter of the linear that produced ``h``, given
    exactly when ``fused_dbias`` said so for that linear (which then ran with
    the bias detached); its gradient comes out of this op's backward."""
    hip = dispatch.use_hip(h, "glu")
    if bias is not None and not hip:
        raise RuntimeError("glu_gelu: bias needs the HIP kernel to deliver "
                           "its gradient (see fused_dbias)")
    if hip:
        return _GluGeluFn.apply(h, bias)
    return reference.glu_gelu(h)


class _GeluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h):
        C = dispatch.ext()
        y = C.gelu_fwd(h)
        ctx.save_for_backward(h)
        return y

    @staticmethod
    def backward(ctx, dy):
        (h,) = ctx.saved_tensors
        C = dispatch.ext()
        return C.gelu_bwd(dy.contiguous(), h)


def gelu(h: torch.Tensor) -> torch.Tensor:
    if dispatch.use_hip(h, "glu"):
        return _GeluFn.apply(h)
    return reference.gelu(h)


# ---------------------------------------------------------------------------
# masked cross-entropy (fused log_softmax + NLL gather; mask math on host)
# ---------------------------------------------------------------------------

class _CERowFn(torch.autograd.Function):
    """Per-row fused -log_softmax(logits)[target]; returns nll (B, N) fp32.

    The EOS/pad mask reduction (reference: utils.py:54-59) is cheap
    (B, N)-shaped tensor math and stays in torch; the (B, N, V) work is
    the kernel."""

    @staticmethod
    def forward(ctx, logits, targets):
        C = dispatch.ext()
        nll, lse = C.ce_fwd(logits, targets)
        ctx.save_for_backward(logits, targets, lse)
        return nll

    @staticmethod
    def backward(ctx, dnll):
        logits, targets, lse = ctx.saved_tensors
        C = dispatch.ext()
        dlogits = C.ce_bwd(dnll.contiguous(), logits, targets, lse)
        return dlogits, None


def cross_entropy(logits: torch.Tensor, targets: torch.Tensor,
                  ignore_index: int = 0) -> torch.Tensor:
    """Masked CE with first-pad-as-EOS (reference: utils.py:45-59); the
    per-sequence masked mean then batch mean reduction order is preserved
    (reference: utils.py:67,75-76)."""
    if dispatch.use_hip(logits, "ce"):
        targets = targets.long().contiguous()
        nll = _CERowFn.apply(logits.contiguous(), targets)
        mask = targets != ignore_index
        eos_mask = (~mask).long().cumsum(dim=-1) == 1
        mask = (mask | eos_mask).to(nll.dtype)
        ce_per_seq = (nll * mask).sum(dim=-1) / mask.sum(dim=-1)
        return ce_per_seq.mean()
    return reference.cross_entropy(logits, targets, ignore_index)


# ---------------------------------------------------------------------------
# SGU spatial gating
# ---------------------------------------------------------------------------

_TRI_CACHE = {}


def _tri_tiles(n: int, device) -> tuple:
    """Lower-triangle 64x64 tile index lists for sgu_dw (cached per n)."""
    key = (n, str(device))
    if key not in _TRI_CACHE:
        ms, ks = [], []
        for mt in range(n // 64):
            for kt in range(mt + 1):
                ms.append(mt)
                ks.append(kt)
        _TRI_CACHE[key] = (
            torch.tensor(ms, dtype=torch.int32, device=device),
            torch.tensor(ks, dtype=torch.int32, device=device),
        )
    return _TRI_CACHE[key]


class _SGUFn(torch.autograd.Function):
    """Causal spatial matmul + bias + gate multiply on the hand-written
    CDNA4 kernels (ops/hip/sgu.hip)."""

    @staticmethod
    def forward(ctx, xa, g_ln, w, bias):
        C = dispatch.ext()
        out, gate_out = C.sgu_fwd(xa, g_ln, w, bias)
        ctx.save_for_backward(xa, g_ln, w, gate_out)
        return out

    @staticmethod
    def backward(ctx, dy):
        xa, g_ln, w, gate_out = ctx.saved_tensors
        C = dispatch.ext()
        dy = dy.contiguous()
        dxa = dy * gate_out
        t = (dy * xa).contiguous()
        dg_ln = C.sgu_dgate(t, w)
        n = xa.shape[1]
        tri_m, tri_k = _tri_tiles(n, xa.device)
        dw = C.sgu_dw(t, g_ln, tri_m, tri_k).to(w.dtype)
        db = t.float().sum(dim=(0, 2)).unsqueeze(-1).to(w.dtype)
        return dxa, dg_ln, dw, db


def sgu_gate(x: torch.Tensor, norm_weight: torch.Tensor,
             spatial_weights: torch.Tensor, spatial_biases: torch.Tensor,
             eps: float = 1e-5) -> torch.Tensor:
    """gMLP spatial gating unit core (reference: progen.py:166-183).

    GPU path: fused LN kernel on the gate half + the hand-written causal
    spatial-matmul kernels (ops/hip/sgu.hip — the tril mask is baked into
    the tile iteration). Sequences shorter than 256 (toy configs) use the
    hipBLASLt composite path."""
    if dispatch.use_hip(x, "sgu"):
        xa, gate = x.chunk(2, dim=-1)
        gate_ln = ln_shift(gate.contiguous(), norm_weight, shift=False, eps=eps)
        n = x.shape[1]
        d = xa.shape[-1]
        if (x.dtype == torch.bfloat16 and n % 256 == 0 and d % 64 == 0):
            w = spatial_weights[:n, :n].contiguous()
            return _SGUFn.apply(xa.contiguous(), gate_ln, w,
                                spatial_biases[:n])
        w = spatial_weights[:n, :n].tril().to(gate_ln.dtype)
        gate_ln = torch.einsum("bnd,mn->bmd", gate_ln, w) + \
            spatial_biases[:n].to(gate_ln.dtype)
        return xa * gate_ln
    return reference.sgu_gate(x, norm_weight, spatial_weights, spatial_biases, eps)


# ---------------------------------------------------------------------------
# fused decode-step ops (inference only; progen_amd._C_decode)
# ---------------------------------------------------------------------------
# One row per batch element, caches updated in place, the position read
# from a 0-dim int64 device tensor — see decode.forward_step_fused. No
# autograd: the decode step runs under no_grad.

def decode_ln_shift(h: torch.Tensor, res, weight: torch.Tensor, prev,
                    shift: bool = True, eps: float = 1e-5) -> torch.Tensor:
    """h <- h + res (in place); y = shift(LN(h) * weight) with the shifted
    half taken from ``prev``; prev <- LN row (in place). Returns y."""
    if dispatch.use_hip(h, "dec_ln"):
        return dispatch.ext_decode().dec_ln_shift(
            h, res, weight, prev, bool(shift), float(eps))
    return reference.decode_ln_shift(h, res, weight, prev, shift, eps)


def decode_attention(qkv: torch.Tensor, sin: torch.Tensor, cos: torch.Tensor,
                     pos: torch.Tensor, k_cache: torch.Tensor,
                     v_cache: torch.Tensor, window_size: int) -> torch.Tensor:
    """Rotary on q, k and v at row ``pos``, cache write, one attention row
    over the local band (reference.decode_attention)."""
    if dispatch.use_hip(qkv, "dec_attn"):
        return dispatch.ext_decode().dec_attn(
            qkv, sin, cos, pos, k_cache, v_cache, int(window_size))
    return reference.decode_attention(qkv, sin, cos, pos, k_cache, v_cache,
                                      window_size)


def decode_sgu(h: torch.Tensor, norm_weight: torch.Tensor,
               hist: torch.Tensor, spatial_weights: torch.Tensor,
               spatial_biases: torch.Tensor, pos: torch.Tensor,
               eps: float = 1e-5) -> torch.Tensor:
    """Gate LN, history write at row ``pos`` and the causal spatial row of
    the SGU (reference.decode_sgu)."""
    if dispatch.use_hip(h, "dec_sgu"):
        return dispatch.ext_decode().dec_sgu(
            h, norm_weight, hist, spatial_weights, spatial_biases, pos,
            float(eps))
    return reference.decode_sgu(h, norm_weight, hist, spatial_weights,
                                spatial_biases, pos, eps)


# ---------------------------------------------------------------------------
# decode-step linear with fused epilogue (progen_amd._C_decode_linear)
# ---------------------------------------------------------------------------

DEC_LINEAR_ACTS = ("none", "gelu", "glu")
# the kernel's own limit on rows (ops/hip/decode_linear_kernels.h)
DEC_LINEAR_KERNEL_MAX_B = 32
# largest batch the routing sends to the kernel, set by the end-to-end
# measurement of profiles/decode_linear.md (the step wins at 1, 8 and 16
# rows and loses at 32); above it hipBLASLt runs
DEC_LINEAR_MAX_B = 16


def decode_linear_supported(B: int, K: int, N: int, act: str, dtype) -> bool:
    """True when ``decode_linear`` routes a (B, K) x (N, K) call of ``dtype``
    with ``act`` to the HIP kernel (given a GPU tensor): the kernel's
    contract, and the routing limit ``DEC_LINEAR_MAX_B``."""
    if act not in DEC_LINEAR_ACTS:
        return False
    if dtype not in (torch.bfloat16, torch.float32):
        return False
    if not 1 <= B <= min(DEC_LINEAR_MAX_B, DEC_LINEAR_KERNEL_MAX_B):
        return False
    if K < 64 or K % 64 != 0:
        return False
    return N >= 16 and N % (32 if act == "glu" else 16) == 0


def decode_linear(x: torch.Tensor, w: torch.Tensor, bias=None,
                  act: str = "none") -> torch.Tensor:
    """act(x @ w^T + bias) for the (B, K) rows of a decode step
    (reference.decode_linear). On a GPU a supported shape runs the HIP
    kernel, which adds the bias and applies the activation on its fp32
    accumulators; any other shape is a plain GEMM and goes to hipBLASLt
    like every other one, followed by the GLU/GELU kernel."""
    if act not in DEC_LINEAR_ACTS:
        raise ValueError(f"decode_linear: unknown act {act!r}")
    if dispatch.use_hip(x, "dec_linear") and x.dim() == 2 and w.dim() == 2 \
            and x.dtype == w.dtype \
            and decode_linear_supported(x.shape[0], x.shape[1], w.shape[0],
                                        act, x.dtype):
        return dispatch.ext_decode_linear().dec_linear(
            x.contiguous(), w.contiguous(),
            None if bias is None else bias.contiguous(), act)
    h = F.linear(x, w, bias)
    if act == "glu":
        return glu_gelu(h)
    if act == "gelu":
        return gelu(h)
    return h


# ---------------------------------------------------------------------------
# prefill of the decode caches (inference only; progen_amd._C_prefill)
# ---------------------------------------------------------------------------
# The full-sequence attention and SGU ops over a (B, Np) prime, which also
# leave rows [0, P) of the decode caches as P decode steps would have — see
# decode.prefill. ``P`` is a host int; no autograd. ``admit``, a (B, 2) int64
# device tensor of [slot, rows] per batch row, sends batch row b's rows
# [0, min(rows, P)) to row ``slot`` of caches of any number of rows instead,
# and nowhere when the slot is out of range — see decode.prefill_rows.

def prefill_attention(qkv: torch.Tensor, sin: torch.Tensor, cos: torch.Tensor,
                      heads: int, window_size: int, k_cache: torch.Tensor,
                      v_cache: torch.Tensor, P: int,
                      admit=None) -> torch.Tensor:
    """``local_attention`` of qkv (B, Np, 3*H*dh) that also stores the rotated
    k and v of rows < P into the (B, H, Nc, dh) caches
    (reference.prefill_attention). ``sin``/``cos`` hold at least Np rows. On
    a GPU the rotation and the cache write are one HIP kernel and the
    attention is ``attn_fwd``, bf16 only."""
    if dispatch.use_hip(qkv, "prefill_kv"):
        qkv_rot = dispatch.ext_prefill().prefill_rope_kv(
            qkv.contiguous(), sin, cos, k_cache, v_cache, int(P), admit)
        out, _lse = dispatch.ext().attn_fwd(qkv_rot, int(heads),
                                            int(window_size))
        return out
    return reference.prefill_attention(qkv, sin, cos, heads, window_size,
                                       k_cache, v_cache, int(P), admit)


def prefill_sgu(x: torch.Tensor, norm_weight: torch.Tensor,
                spatial_weights: torch.Tensor, spatial_biases: torch.Tensor,
                hist: torch.Tensor, P: int, eps: float = 1e-5,
                admit=None) -> torch.Tensor:
    """``sgu_gate`` of x (B, Np, 2*d2) that also stores the LN'd gate rows
    < P into the (B, Nc, d2) history (reference.prefill_sgu). On a GPU the
    gate LN reads its half of ``x`` in place and writes the history in the
    same HIP kernel, and the spatial matmul is ``sgu_fwd``: bf16,
    Np % 256 == 0 and d2 % 64 == 0, or the kernels raise."""
    if dispatch.use_hip(x, "prefill_gate"):
        gate_ln = dispatch.ext_prefill().prefill_gate_ln(
            x.contiguous(), norm_weight, hist, int(P), float(eps), admit)
        n = x.shape[1]
        xa = x[..., :x.shape[-1] // 2].contiguous()
        out, _gate_out = dispatch.ext().sgu_fwd(
            xa, gate_ln, spatial_weights[:n, :n].contiguous(),
            spatial_biases[:n])
        return out
    return reference.prefill_sgu(x, norm_weight, spatial_weights,
                                 spatial_biases, hist, int(P), eps, admit)


# ---------------------------------------------------------------------------
# decode-step sampler (progen_amd._C_decode_sample)
# ---------------------------------------------------------------------------

# the kernel stages a whole row per workgroup (ops/hip/decode_sample_kernels.h)
DEC_SAMPLE_MAX_V = 1024


def decode_sample(logits: torch.Tensor, pos: torch.Tensor, seed: torch.Tensor,
                  seq: torch.Tensor, lens: torch.Tensor, pads: torch.Tensor,
                  token: torch.Tensor, top_k: int = 0, greedy: bool = False,
                  u_out=None) -> None:
    """Sample position pos + 1 of every row into ``seq``, ``pads`` and
    ``token``, in place (reference.decode_sample): argmax when ``greedy``,
    else gumbel-max over the strict top-k (``top_k`` 0: the whole row) with
    Philox noise keyed by ``seed``. On a GPU this is the HIP kernel, which a
    graph can capture; a vocabulary it does not serve is an error there,
    never a fall-back."""
    if dispatch.use_hip(logits, "dec_sample"):
        dispatch.ext_decode_sample().dec_sample(
            logits, pos, seed, seq, lens, pads, token, int(top_k),
            bool(greedy), u_out)
        return
    reference.decode_sample(logits, pos, seed, seq, lens, pads, token,
                            top_k, greedy, u_out)


# ---------------------------------------------------------------------------
# slot decode-step ops (inference only; progen_amd._C_decode_slots)
# ---------------------------------------------------------------------------
# The four ops above with one position per batch row: ``pos`` is a (B,)
# int64 device tensor and pos[b] < 0 marks an idle row, which changes
# nothing and gets a zero output row — see decode.forward_step_slots and
# progen_amd/engine.py. They answer to the routing tags of their twins.

def decode_ln_shift_slots(h: torch.Tensor, res, weight: torch.Tensor, prev,
                          pos: torch.Tensor, shift: bool = True,
                          eps: float = 1e-5) -> torch.Tensor:
    """``decode_ln_shift`` per row; a row at position 0 shifts in zeros
    instead of ``prev`` (reference.decode_ln_shift_slots)."""
    if dispatch.use_hip(h, "dec_ln"):
        return dispatch.ext_decode_slots().dec_ln_shift_slots(
            h, res, weight, prev, pos, bool(shift), float(eps))
    return reference.decode_ln_shift_slots(h, res, weight, prev, pos, shift,
                                           eps)


def decode_attention_slots(qkv: torch.Tensor, sin: torch.Tensor,
                           cos: torch.Tensor, pos: torch.Tensor,
                           k_cache: torch.Tensor, v_cache: torch.Tensor,
                           window_size: int) -> torch.Tensor:
    """``decode_attention`` with row b at position pos[b]
    (reference.decode_attention_slots)."""
    if dispatch.use_hip(qkv, "dec_attn"):
        return dispatch.ext_decode_slots().dec_attn_slots(
            qkv, sin, cos, pos, k_cache, v_cache, int(window_size))
    return reference.decode_attention_slots(qkv, sin, cos, pos, k_cache,
                                            v_cache, window_size)


def decode_sgu_slots(h: torch.Tensor, norm_weight: torch.Tensor,
                     hist: torch.Tensor, spatial_weights: torch.Tensor,
                     spatial_biases: torch.Tensor, pos: torch.Tensor,
                     eps: float = 1e-5) -> torch.Tensor:
    """``decode_sgu`` with row b at position pos[b]
    (reference.decode_sgu_slots)."""
    if dispatch.use_hip(h, "dec_sgu"):
        return dispatch.ext_decode_slots().dec_sgu_slots(
            h, norm_weight, hist, spatial_weights, spatial_biases, pos,
            float(eps))
    return reference.decode_sgu_slots(h, norm_weight, hist, spatial_weights,
                                      spatial_biases, pos, eps)


# columns of the slot sampler's per-row controls
SLOT_CTL = ("len", "limit", "top_k", "seed", "stream")


def decode_sample_slots(logits: torch.Tensor, pos: torch.Tensor,
                        token: torch.Tensor, seq: torch.Tensor,
                        pads: torch.Tensor, ctl: torch.Tensor,
                        u_out=None) -> None:
    """Sample position pos[b] + 1 of every live row under its own controls
    ``ctl[b] = [len, limit, top_k, seed, stream]`` into ``seq``, ``pads`` and
    ``token``, and advance or retire the row in ``pos``, all in place
    (reference.decode_sample_slots). On a GPU this is the HIP kernel, which a
    graph can capture; a vocabulary it does not serve is an error there,
    never a fall-back."""
    if dispatch.use_hip(logits, "dec_sample"):
        dispatch.ext_decode_slots().dec_sample_slots(
            logits, pos, token, seq, pads, ctl, u_out)
        return
    reference.decode_sample_slots(logits, pos, token, seq, pads, ctl, u_out)
