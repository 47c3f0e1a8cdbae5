"""Cached incremental decoding (serving path).

The reference's sampler (reference: progen_transformer/utils.py:106-135)
re-runs a full-length forward per emitted token — O(L * N^2). This module
maintains per-layer recurrent state so each new token costs one O(window)
attention row, one O(n) SGU row and the per-token GEMV projections:

  - token shift needs the previous position's LN'd row (progen.py:43-46);
  - windowed attention needs the rotated k/v of the current + previous
    window only (progen.py:88-96) — window 0's zero lookback keys enter
    the softmax denominator unmasked, which the step reproduces exactly;
  - the SGU gate row m is sum_{n<=m} W[m,n]*gate_ln[n] + b[m]
    (progen.py:179-182), so the LN'd gate history is the cache.

Emitted tokens are identical to ``utils.sample`` up to fp reduction-order
noise (tests/test_decode.py pins exact token equality on seeded fp32
models). This is the O(1)-per-token analog of a KV cache for this
architecture; ``sample_cached`` mirrors the sampler quirks (strict-> top-k
with zeros-not-inf, gumbel-max, zero-after-second-pad).
"""

from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F

from .models.progen import ProGenBase
from .ops import functional as OF
from .ops import reference as R


def _ln_row(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """Scale-only LN of a (B, D) row (progen.py:22); stats in fp32."""
    return R.layernorm_nobias(x.unsqueeze(1), weight, eps).squeeze(1)


def _shift_row(y: torch.Tensor, prev: Optional[torch.Tensor]) -> torch.Tensor:
    """Token shift at one position: first ceil(D/2) channels come from the
    PREVIOUS position's LN'd row (zeros at position 0)  (progen.py:43-46)."""
    d = y.shape[-1]
    split = -(-d // 2)
    head = torch.zeros_like(y[..., :split]) if prev is None else prev[..., :split]
    return torch.cat((head, y[..., split:]), dim=-1)


class DecodeCache:
    """Recurrent state for one ``ProGenBase`` forward, batch-first (B, ...).

    Buffers are allocated once at ``seq_len`` capacity (288 GB HBM3E makes
    full-length caches the right trade on MI355X — no ring-buffer
    bookkeeping on the hot path)."""

    def __init__(self, model: ProGenBase, batch: int = 1,
                 device=None, dtype=None):
        cfg = model.cfg
        p = next(model.parameters())
        device = p.device if device is None else device
        dtype = p.dtype if dtype is None else dtype
        self.cfg = cfg
        self.pos = 0
        N, H, DH = cfg.seq_len, cfg.heads, cfg.dim_head
        self.k = []    # per attn layer: (B, H, N, DH) rotated keys
        self.v = []
        # previous position's LN row per branch (token-shift halo);
        # preallocated + written in place so a captured static step
        # updates fixed buffers (zeros == the position-0 "no previous
        # row" semantics)
        self.attn_prev = [torch.zeros(batch, cfg.dim, device=device,
                                      dtype=dtype) for _ in range(cfg.depth)]
        self.ff_prev = [torch.zeros(batch, cfg.dim, device=device,
                                    dtype=dtype) for _ in range(cfg.depth)]
        self.gate_hist = []  # per SGU layer: (B, N, d2) LN'd gate rows
        for _attn, ff in model.layers:
            self.k.append(torch.zeros(batch, H, N, DH, device=device, dtype=dtype))
            self.v.append(torch.zeros(batch, H, N, DH, device=device, dtype=dtype))
            if ff.sgu is not None:
                d2 = ff.sgu.norm_weight.shape[0]
                self.gate_hist.append(
                    torch.zeros(batch, N, d2, device=device, dtype=dtype))
            else:
                self.gate_hist.append(None)


def _attn_step(attn, x, sin_p, cos_p, cache: DecodeCache, li: int) -> torch.Tensor:
    """One LocalAttention row at position cache.pos. x: (B, dim)."""
    p = cache.pos
    H, DH, wsz = attn.heads, cache.cfg.dim_head, attn.window_size
    y = _ln_row(x, attn.norm_weight)
    y_in = _shift_row(y, cache.attn_prev[li]) if attn.shift_tokens else y
    cache.attn_prev[li].copy_(y)
    qkv = F.linear(y_in, attn.to_qkv.weight)            # (B, 3*H*DH)
    B = qkv.shape[0]
    q, k, v = qkv.view(B, 3, H, DH).unbind(1)
    # interleaved rotary on q, k AND v at position p (progen.py:87)
    sc, ss = cos_p.to(q.dtype), sin_p.to(q.dtype)
    q, k, v = (t * sc + R.rotate_every_two(t) * ss for t in (q, k, v))
    cache.k[li][:, :, p] = k
    cache.v[li][:, :, p] = v

    win = p // wsz
    start = (win - 1) * wsz if win > 0 else 0
    keys = cache.k[li][:, :, start:p + 1]               # (B, H, n, DH)
    vals = cache.v[li][:, :, start:p + 1]
    s = torch.einsum("bhd,bhnd->bhn", q, keys) * (DH ** -0.5)
    if win == 0:
        # window 0's zero lookback keys are UNMASKED (progen.py:90-96):
        # wsz extra zero logits in the softmax, zero values
        s = F.pad(s, (wsz, 0))
    s = s - s.amax(dim=-1, keepdim=True)
    a = s.softmax(dim=-1)
    if win == 0:
        a = a[..., wsz:]
    out = torch.einsum("bhn,bhnd->bhd", a, vals).reshape(B, H * DH)
    return F.linear(out, attn.to_out.weight, attn.to_out.bias)


def _ff_step(ff, x, cache: DecodeCache, li: int) -> torch.Tensor:
    """One FeedForward row at position cache.pos. x: (B, dim)."""
    y = _ln_row(x, ff.norm_weight)
    y_in = _shift_row(y, cache.ff_prev[li]) if ff.shift_tokens else y
    cache.ff_prev[li].copy_(y)
    h = F.linear(y_in, ff.proj_in.weight, ff.proj_in.bias)
    if ff.glu:
        a, g = h.chunk(2, dim=-1)
        h = a * F.gelu(g, approximate="tanh")
    else:
        h = F.gelu(h, approximate="tanh")
    if ff.sgu is not None:
        p = cache.pos
        xa, gate = h.chunk(2, dim=-1)
        gate_ln = _ln_row(gate, ff.sgu.norm_weight)
        hist = cache.gate_hist[li]
        hist[:, p] = gate_ln
        w_row = ff.sgu.spatial_weights[p, :p + 1]       # causal row (progen.py:179)
        gate_out = torch.einsum("n,bnd->bd", w_row.to(hist.dtype),
                                hist[:, :p + 1]) + ff.sgu.spatial_biases[p]
        h = xa * gate_out
        h = F.linear(h, ff.sgu.proj_out.weight, ff.sgu.proj_out.bias)
    return F.linear(h, ff.proj_out.weight, ff.proj_out.bias)


@torch.no_grad()
def forward_step(model: ProGenBase, token: torch.Tensor,
                 cache: DecodeCache) -> torch.Tensor:
    """Advance the cache by one token; returns (B, V) logits at this
    position — identical (up to fp noise) to row ``cache.pos`` of a full
    ``model(seq)`` forward over the same prefix."""
    p = cache.pos
    assert p < model.cfg.seq_len, "decode past seq_len"
    if model.rotary_sin.dtype != torch.float32:
        sin, cos = R.fixed_pos_embedding(model.cfg.seq_len, model.cfg.dim_head,
                                         device=model.rotary_sin.device)
        model.rotary_sin, model.rotary_cos = sin, cos
    sin_p, cos_p = model.rotary_sin[p], model.rotary_cos[p]
    h = model.embed(token.long().reshape(-1))           # (B, dim)
    for li, (attn, ff) in enumerate(model.layers):
        h = h + _attn_step(attn, h, sin_p, cos_p, cache, li)
        h = h + _ff_step(ff, h, cache, li)
    h = _ln_row(h, model.final_norm_weight)
    logits = F.linear(h, model.to_logits.weight, model.to_logits.bias)
    cache.pos = p + 1
    return logits


@torch.no_grad()
def forward_step_static(model: ProGenBase, token: torch.Tensor,
                        cache: DecodeCache,
                        pos_dev: torch.Tensor) -> torch.Tensor:
    """Position-STATIC decode step: numerically identical to
    ``forward_step`` but every operation has position-independent shapes
    and reads the position from a device tensor — the form a hipGraph
    can capture once and replay per token (TODO.md "Serving"; the
    pure-replay rule of profiles/r01_graph_interleave_bug.md means the
    position increment must itself be in-graph, which this function's
    tensor-only indexing permits).

    Mechanics per layer:
      - attention gathers a FIXED 2*window_size key slice at indices
        win_start - wsz + [0, 2wsz); indices < 0 fetch zeroed k/v and
        stay UNMASKED (exactly the reference's window-0 zero-pad quirk,
        progen.py:90-96); indices > pos are masked -inf;
      - the SGU row uses the full spatial_weights row masked by
        arange(N) <= pos (static O(N*d2) dot);
      - rotary rows, shift halos and cache writes are index_put/gather
        with tensor indices.

    ``pos_dev``: 0-dim int64 tensor holding the current position; the
    caller increments it AFTER the step (in-graph when captured).
    Updates the same ``DecodeCache`` as ``forward_step``."""
    cfg = model.cfg
    wsz = cfg.window_size
    dev = token.device
    p = pos_dev  # 0-dim int64 on device
    sin_p = model.rotary_sin.index_select(0, p.reshape(1))[0]
    cos_p = model.rotary_cos.index_select(0, p.reshape(1))[0]
    h = model.embed(token.long().reshape(-1))

    win_start = (p // wsz) * wsz
    gather_idx = win_start - wsz + torch.arange(2 * wsz, device=dev)
    valid = (gather_idx >= 0)                       # zero-halo quirk keys
    causal = (gather_idx <= p)                      # future keys masked
    safe_idx = gather_idx.clamp(min=0)

    for li, (attn, ff) in enumerate(model.layers):
        # ---- attention branch ----
        x = h
        y = _ln_row(x, attn.norm_weight)
        y_in = _shift_row(y, cache.attn_prev[li]) if attn.shift_tokens else y
        cache.attn_prev[li].copy_(y)
        qkv = F.linear(y_in, attn.to_qkv.weight)
        B = qkv.shape[0]
        H, DH = attn.heads, cfg.dim_head
        q, k, v = qkv.view(B, 3, H, DH).unbind(1)
        sc, ss = cos_p.to(q.dtype), sin_p.to(q.dtype)
        q, k, v = (t * sc + R.rotate_every_two(t) * ss for t in (q, k, v))
        cache.k[li].index_copy_(2, p.reshape(1), k.unsqueeze(2))
        cache.v[li].index_copy_(2, p.reshape(1), v.unsqueeze(2))
        keys = cache.k[li].index_select(2, safe_idx)    # (B, H, 2wsz, DH)
        vals = cache.v[li].index_select(2, safe_idx)
        kmask = valid.view(1, 1, -1, 1).to(keys.dtype)
        keys = keys * kmask                             # zero halo keys
        vals = vals * kmask
        s_row = torch.einsum("bhd,bhnd->bhn", q, keys) * (DH ** -0.5)
        # masked_fill with a python scalar: no host->device transfer, so
        # the op is hipGraph-capturable (torch.tensor(scalar) is not)
        s_row = s_row.masked_fill(~causal.view(1, 1, -1), -1e30)
        s_row = s_row - s_row.amax(dim=-1, keepdim=True)
        a = s_row.softmax(dim=-1)
        out = torch.einsum("bhn,bhnd->bhd", a, vals).reshape(B, H * DH)
        h = h + F.linear(out, attn.to_out.weight, attn.to_out.bias)

        # ---- ff branch ----
        y = _ln_row(h, ff.norm_weight)
        y_in = _shift_row(y, cache.ff_prev[li]) if ff.shift_tokens else y
        cache.ff_prev[li].copy_(y)
        t = F.linear(y_in, ff.proj_in.weight, ff.proj_in.bias)
        if ff.glu:
            a2, g2 = t.chunk(2, dim=-1)
            t = a2 * F.gelu(g2, approximate="tanh")
        else:
            t = F.gelu(t, approximate="tanh")
        if ff.sgu is not None:
            sgu = ff.sgu
            xa, gate = t.chunk(2, dim=-1)
            gate_ln = _ln_row(gate, sgu.norm_weight)
            hist = cache.gate_hist[li]
            hist.index_copy_(1, p.reshape(1), gate_ln.unsqueeze(1))
            n = hist.shape[1]
            w_row = sgu.spatial_weights.index_select(0, p.reshape(1))[0, :n]
            past = (torch.arange(n, device=dev) <= p).to(hist.dtype)
            gate_out = torch.einsum("n,bnd->bd", w_row.to(hist.dtype) * past,
                                    hist) + \
                sgu.spatial_biases.index_select(0, p.reshape(1))[0]
            t = xa * gate_out
            t = F.linear(t, sgu.proj_out.weight, sgu.proj_out.bias)
        h = h + F.linear(t, ff.proj_out.weight, ff.proj_out.bias)

    y = _ln_row(h, model.final_norm_weight)
    return F.linear(y, model.to_logits.weight, model.to_logits.bias)
    # NOTE: cache.pos is NOT advanced — the caller owns pos_dev and
    # increments it (in-graph when captured)


@torch.no_grad()
def forward_step_fused(model: ProGenBase, token: torch.Tensor,
                       cache: DecodeCache,
                       pos_dev: torch.Tensor,
                       fused_linear: bool = False) -> torch.Tensor:
    """Decode step on the fused decode kernels: same contract as
    ``forward_step_static`` (position from the 0-dim int64 ``pos_dev``,
    same ``DecodeCache``, position NOT advanced), but every non-GEMM op of
    a branch is one of three ops — ``OF.decode_ln_shift``,
    ``OF.decode_attention``, ``OF.decode_sgu`` (ops/hip/decode_*.hip on a
    GPU, ops/reference.py on CPU) — plus the existing GLU/GELU kernel.
    By the code that is 8 launches per GLU layer and 10 per SGU layer.

    The branch output is carried into the next ``decode_ln_shift`` as its
    residual, as in ``ProGenBase.forward``; the final norm consumes the
    last one. No workgroup of any kernel waits on another, so the step is
    as capturable and replayable as the static one.

    ``fused_linear=True`` sends the six projections and the logits head
    through ``OF.decode_linear`` (ops/hip/decode_linear.hip on a GPU), with
    the bias and the GLU/GELU of ``proj_in`` folded in: 7 launches per GLU
    layer and 9 per SGU layer, and no bias copy. On the CPU it computes
    the same ops as the default, bit for bit."""
    return _fused_step(model, token, cache, pos_dev, fused_linear,
                       slots=False)


@torch.no_grad()
def forward_step_slots(model: ProGenBase, token: torch.Tensor,
                       cache: DecodeCache, pos: torch.Tensor,
                       fused_linear: bool = False) -> torch.Tensor:
    """``forward_step_fused`` with one position per batch row: ``pos`` is a
    (B,) int64 device tensor and row b of the same ``DecodeCache`` advances
    at pos[b]. A row with pos[b] < 0 is idle: none of its cache rows, shift
    halos or histories change, and it flows through the projections as
    zeros. A row at position 0 starts on a clean slate whatever its cache
    row still holds from an earlier request: its token shift reads zeros and
    the attention band and the SGU prefix only ever reach rows the request
    wrote itself. Positions are NOT advanced here — ``OF.decode_sample_slots``
    does that, and retires finished rows. Same ops and launch counts as
    ``forward_step_fused``, on the slot kernels (ops/hip/decode_slots.hip on
    a GPU, ops/reference.py on CPU)."""
    return _fused_step(model, token, cache, pos, fused_linear, slots=True)


def _fused_step(model: ProGenBase, token: torch.Tensor, cache: DecodeCache,
                pos_dev: torch.Tensor, fused_linear: bool,
                slots: bool) -> torch.Tensor:
    """The layer loop of ``forward_step_fused`` (``pos_dev`` 0-dim) and
    ``forward_step_slots`` (``pos_dev`` (B,)): the two differ only in which
    set of ops reads the position."""
    cfg = model.cfg
    if slots:
        def ln_shift(h, r, weight, prev, shift):
            return OF.decode_ln_shift_slots(h, r, weight, prev, pos_dev,
                                            shift=shift)
        attention, sgu_row = OF.decode_attention_slots, OF.decode_sgu_slots
    else:
        def ln_shift(h, r, weight, prev, shift):
            return OF.decode_ln_shift(h, r, weight, prev, shift=shift)
        attention, sgu_row = OF.decode_attention, OF.decode_sgu
    if fused_linear:
        def linear(x, lin, act="none"):
            return OF.decode_linear(x, lin.weight, lin.bias, act)
    else:
        def linear(x, lin, act="none"):
            y = F.linear(x, lin.weight, lin.bias)
            if act == "glu":
                return OF.glu_gelu(y)
            return OF.gelu(y) if act == "gelu" else y
    if model.rotary_sin.dtype != torch.float32:
        sin, cos = R.fixed_pos_embedding(cfg.seq_len, cfg.dim_head,
                                         device=model.rotary_sin.device)
        model.rotary_sin, model.rotary_cos = sin, cos
    sin, cos = model.rotary_sin, model.rotary_cos
    h = model.embed(token.long().reshape(-1))           # (B, dim), updated in place
    r = None
    for li, (attn, ff) in enumerate(model.layers):
        y = ln_shift(h, r, attn.norm_weight, cache.attn_prev[li],
                     attn.shift_tokens)
        qkv = linear(y, attn.to_qkv)
        out = attention(qkv, sin, cos, pos_dev, cache.k[li], cache.v[li],
                        attn.window_size)
        a = linear(out, attn.to_out)

        y = ln_shift(h, a, ff.norm_weight, cache.ff_prev[li],
                     ff.shift_tokens)
        t = linear(y, ff.proj_in, "glu" if ff.glu else "gelu")
        if ff.sgu is not None:
            sgu = ff.sgu
            t = sgu_row(t, sgu.norm_weight, cache.gate_hist[li],
                        sgu.spatial_weights, sgu.spatial_biases, pos_dev)
            t = linear(t, sgu.proj_out)
        r = linear(t, ff.proj_out)
    y = ln_shift(h, r, model.final_norm_weight, None, False)
    return linear(y, model.to_logits)


# shortest prime the callers route to ``prefill`` on a GPU, from the
# time-to-first-token measurement of profiles/decode_prefill.md: on the
# flagship the forward loses to the step loop at 2 and 3 tokens, ties at 4
# and wins from 7 (batch 8) and 8 (batch 1)
PREFILL_MIN_TOKENS = 8


def _prefill_len(model: ProGenBase, P: int, device) -> int:
    """Rows of the forward that prefills P positions: P padded up to what
    the full-sequence ops take. The reference ops want whole windows;
    the GPU's ``sgu_fwd`` also wants multiples of 256 rows."""
    L = model.cfg.window_size
    if torch.device(device).type == "cuda" and \
            any(ff.sgu is not None for _attn, ff in model.layers):
        L = math.lcm(L, 256)
    return -(-P // L) * L


def prefill_supported(model: ProGenBase, P: int, device) -> bool:
    """True when the samplers prefill a P-token prime on ``device`` with one
    forward (``prefill``) instead of P decode steps. On the CPU that is
    whenever the padded prime fits the model; on a GPU it also takes what
    the kernels serve (bf16, dim_head 64, window and SGU width multiples of
    64) and a prime of at least ``PREFILL_MIN_TOKENS``."""
    cfg = model.cfg
    device = torch.device(device)
    if not 1 <= P <= cfg.seq_len or \
            _prefill_len(model, P, device) > cfg.seq_len:
        return False
    if device.type != "cuda":
        return True
    return next(model.parameters()).dtype == torch.bfloat16 \
        and cfg.dim_head == 64 and cfg.window_size % 64 == 0 \
        and all(ff.sgu is None or ff.sgu.norm_weight.shape[0] % 64 == 0
                for _attn, ff in model.layers) \
        and P >= PREFILL_MIN_TOKENS


def _rotary_fp32(model: ProGenBase):
    """The model's rotary tables as the kernels read them, fp32."""
    if model.rotary_sin.dtype != torch.float32:
        sin, cos = R.fixed_pos_embedding(model.cfg.seq_len,
                                         model.cfg.dim_head,
                                         device=model.rotary_sin.device)
        model.rotary_sin, model.rotary_cos = sin, cos
    return model.rotary_sin, model.rotary_cos


def _prefill_layers(model: ProGenBase, h: torch.Tensor, cache: DecodeCache,
                    P: int, admit: Optional[torch.Tensor], halo):
    """The layer loop of ``prefill`` and ``prefill_rows`` over the embedded
    (B, Np, dim) rows ``h``: ``ProGenBase.forward``'s, with the cache writes
    of ``OF.prefill_attention`` / ``OF.prefill_sgu`` (rows < P, and where
    ``admit`` says when given) and ``halo(stream, weight, prev)`` storing the
    token-shift halo of each branch. Returns the residual stream and the last
    branch output, not yet added."""
    sin, cos = _rotary_fp32(model)
    r = None
    for li, (attn, ff) in enumerate(model.layers):
        y, h = OF.ln_shift_res(h, r, attn.norm_weight,
                               shift=attn.shift_tokens)
        halo(h, attn.norm_weight, cache.attn_prev[li])
        qkv = F.linear(y, attn.to_qkv.weight)
        out = OF.prefill_attention(qkv, sin, cos, attn.heads,
                                   attn.window_size, cache.k[li],
                                   cache.v[li], P, admit=admit)
        a = F.linear(out, attn.to_out.weight, attn.to_out.bias)

        y, h = OF.ln_shift_res(h, a, ff.norm_weight, shift=ff.shift_tokens)
        halo(h, ff.norm_weight, cache.ff_prev[li])
        t = F.linear(y, ff.proj_in.weight, ff.proj_in.bias)
        t = OF.glu_gelu(t) if ff.glu else OF.gelu(t)
        if ff.sgu is not None:
            sgu = ff.sgu
            t = OF.prefill_sgu(t, sgu.norm_weight, sgu.spatial_weights,
                               sgu.spatial_biases, cache.gate_hist[li], P,
                               admit=admit)
            t = F.linear(t, sgu.proj_out.weight, sgu.proj_out.bias)
        r = F.linear(t, ff.proj_out.weight, ff.proj_out.bias)
    return h, r


@torch.no_grad()
def prefill(model: ProGenBase, tokens: torch.Tensor, cache: DecodeCache,
            pos_dev: Optional[torch.Tensor] = None,
            want_logits: bool = False) -> Optional[torch.Tensor]:
    """Fill a fresh ``cache`` for positions [0, P) from ONE forward over the
    (B, P) ``tokens``, instead of P decode steps that each stream every
    weight for a single row.

    The model is causal, so row p of a full forward equals what step p
    computes; the tokens are padded with id 0 to the length the
    full-sequence ops take and rows < P are exact. The layer loop is
    ``ProGenBase.forward``'s, with ``OF.prefill_attention`` and
    ``OF.prefill_sgu`` leaving the rotated k/v and the LN'd gate rows in
    the cache on their way, and plain ``F.linear`` projections as in the
    decode steps. The token-shift halos ``attn_prev``/``ff_prev`` get the
    unshifted LN of row P-1. Cache rows >= P are not touched.

    Afterwards ``cache.pos`` is P, as is ``pos_dev`` (the fused step's
    0-dim int64 device position) when given. ``want_logits``: return the
    (B, V) logits of row P-1, which is all a sampler needs; the final norm
    and the head are skipped for every other row. Eager, so it belongs
    before any graph capture.

    Raises ValueError unless ``tokens`` is (B, P >= 1) for the cache's batch
    and the cache is fresh, IndexError when the padded prime does not fit
    the model's seq_len."""
    cfg = model.cfg
    tokens = torch.as_tensor(tokens)
    if tokens.dim() != 2 or tokens.shape[1] < 1 \
            or tokens.shape[0] != cache.attn_prev[0].shape[0]:
        raise ValueError("prefill: tokens must be (B, P >= 1) with the "
                         f"cache's batch, got {tuple(tokens.shape)}")
    if cache.pos != 0:
        raise ValueError("prefill needs a fresh cache, this one is at "
                         f"position {cache.pos}")
    P = tokens.shape[1]
    dev = cache.attn_prev[0].device
    Np = _prefill_len(model, P, dev)
    if Np > cfg.seq_len:
        raise IndexError(f"prefill of {P} tokens ({Np} padded) past seq_len "
                         f"({cfg.seq_len})")
    last = P - 1

    def halo(s, weight, prev):
        # the decode step's own LN of one row, which also stores it
        return OF.decode_ln_shift(s[:, last].contiguous(), None, weight, prev,
                                  shift=False)

    h = model.embed(F.pad(tokens.long(), (0, Np - P)).to(dev))  # (B, Np, dim)
    h, r = _prefill_layers(model, h, cache, P, None, halo)

    cache.pos = P
    if pos_dev is not None:
        pos_dev.fill_(P)
    if not want_logits:
        return None
    y = OF.decode_ln_shift(h[:, last].contiguous(), r[:, last].contiguous(),
                           model.final_norm_weight, None, shift=False)
    return F.linear(y, model.to_logits.weight, model.to_logits.bias)


@torch.no_grad()
def prefill_rows(model: ProGenBase, tokens: torch.Tensor, cache: DecodeCache,
                 admit: torch.Tensor, src: torch.Tensor,
                 live: torch.Tensor) -> None:
    """``prefill`` for the slot engine: ONE forward over the (R, Np) device
    ``tokens`` that fills, for every batch row r with
    ``admit[r] = [slot, rows]`` and 0 <= slot < S, rows [0, rows) of row
    ``slot`` of the S-row ``cache``, and nothing for any other r. Everything
    it depends on is read from device memory, so a graph can capture it:
    no host value but the shapes, no fill and no logits.

    ``tokens``: int64, Np a length the full-sequence ops take
    (``_prefill_len``), id 0 past each row's prime. ``admit``: (R, 2) int64.
    ``src`` and ``live``, (S,) int64, place the token-shift halos: slot b
    takes the LN of flat row ``src[b]`` (r * Np + rows - 1 for an admitted
    slot, 0 otherwise) of the (R * Np, dim) stream where ``live[b] == 0``
    and keeps its own where ``live[b] == -1`` — one
    ``OF.decode_ln_shift_slots`` per branch, with ``live`` as its positions.
    Each slot is named by at most one batch row. ``cache.pos`` is not used:
    the engine keeps one position per slot."""
    R_, Np = tokens.shape
    D = model.cfg.dim

    def halo(s, weight, prev):
        OF.decode_ln_shift_slots(s.reshape(R_ * Np, D).index_select(0, src),
                                 None, weight, prev, live, shift=False)

    h = model.embed(tokens)                             # (R, Np, dim)
    _prefill_layers(model, h, cache, Np, admit, halo)


def _prefill_if_supported(model: ProGenBase, tokens: torch.Tensor,
                          cache: DecodeCache, pos_dev: Optional[torch.Tensor],
                          want_logits: bool):
    """``prefill`` for the samplers: (True, its result) when
    ``prefill_supported``, else (False, None) and the caller steps through
    the tokens as it would without the flag."""
    dev = cache.attn_prev[0].device
    if tokens.shape[1] < 1 or \
            not prefill_supported(model, tokens.shape[1], dev):
        return False, None
    return True, prefill(model, tokens, cache, pos_dev, want_logits)


def _prefill_common_prefix(model: ProGenBase, seq: torch.Tensor, lens,
                           cache: DecodeCache) -> int:
    """Prefill what every row of a ragged batch has in common: the rows of a
    cache share one position, so that is the first min(lens) - 1 columns of
    ``seq`` (B, length) — every row's next token is then still a prime
    token, and no logits are needed. Returns the position to step on from:
    that count, or 0 when nothing was prefilled."""
    Pc = min(lens) - 1
    done, _ = _prefill_if_supported(model, seq[:, :max(Pc, 0)], cache, None,
                                    False)
    return Pc if done else 0


class DeviceSampler:
    """Sampling state that lives on the model's device, for
    ``OF.decode_sample``: the sequences ``seq`` (B, L), the prime lengths
    ``lens``, the pad counts ``pads`` over written tokens and the Philox
    ``seed`` (1,), all int64.

    Every tensor is initialised by a host-to-device COPY of a host tensor,
    never by a device kernel, so building one between graph replays keeps
    the pure-replay rule. ``top_k`` None is no top-k mask; ``seed`` None is
    greedy argmax, else an int in [0, 2^63). The uniform stream is the
    kernel's own Philox4x32-10 (ops/reference.py, decode_sample_uniform),
    not torch's generator stream. ``written``: how many leading positions
    of ``seq`` are already decided when sampling starts (1, or more after
    a prefill); the pad counts start from those."""

    def __init__(self, seq: torch.Tensor, lens, top_k: Optional[int],
                 seed: Optional[int], device, written: int = 1):
        seq = torch.as_tensor(seq).long().cpu()
        if seq.dim() != 2:
            raise ValueError("DeviceSampler: seq must be (B, L)")
        self.top_k = 0 if top_k is None else int(top_k)
        if self.top_k < 0:
            raise ValueError(f"top_k must be >= 0, got {top_k}")
        self.greedy = seed is None
        if seed is not None and not 0 <= int(seed) < 2 ** 63:
            raise ValueError(f"seed must be in [0, 2^63), got {seed}")
        self.seq = seq.contiguous().to(device, copy=True)  # never the caller's
        self.lens = torch.tensor([int(n) for n in lens],
                                 dtype=torch.long).to(device)
        # the first ``written`` positions are written at entry; the unfilled
        # tail must not count
        self.pads = (seq[:, :written] == 0).sum(dim=-1).to(device)
        self.seed = torch.tensor([0 if seed is None else int(seed)],
                                 dtype=torch.long).to(device)

    def sample(self, logits: torch.Tensor, pos_dev: torch.Tensor,
               token: torch.Tensor) -> None:
        """Sample position pos_dev + 1 into ``seq``, ``pads`` and the (B,)
        int64 ``token`` buffer the next step reads."""
        OF.decode_sample(logits, pos_dev, self.seed, self.seq, self.lens,
                         self.pads, token, self.top_k, self.greedy)


class GraphedDecodeStep:
    """hipGraph-captured decode step (TODO.md "Serving"; VERDICT r1 item
    6): one replay = forward_step_static + in-graph pos_dev increment
    (``fused=True``: forward_step_fused, the decode kernels;
    ``fused_linear=True`` on top of it: its projections on the decode
    linear kernel).
    The eager per-token step is launch-bound (~500 kernel launches); the
    graph replays them as one unit.

    Pure-replay discipline (profiles/r01_graph_interleave_bug.md): no
    eager KERNEL may run between replays. The per-token loop only does
    host<->device MEMCPYs (token in, logits out) and CPU-side sampling,
    which keeps replay state intact — validated by
    tests/test_gpu_decode_graph.py against the eager cached decoder.

    Usage:
        cache = DecodeCache(model, batch=B)
        ... eager prefill via forward_step ...
        g = GraphedDecodeStep(model, cache, start_pos=cache.pos)
        for _ in range(n):
            logits = g.step(tokens)        # (B, V) device tensor
            tokens = <sample on host>      # no device kernels!

    With a ``sampler`` (``DeviceSampler``) the capture also holds
    ``OF.decode_sample``, after the forward and before the position
    advance, writing into the step's own static ``token`` buffer: a replay
    then feeds the next one and ``replay(n)`` runs n steps with nothing
    from the host in between. The kernel is inside the graph, so the
    pure-replay rule holds. Set the first token with
    ``g.token.copy_(host_tokens)`` (a memcpy).
    """

    def __init__(self, model: ProGenBase, cache: DecodeCache,
                 start_pos: int, warmup: int = 2, fused: bool = False,
                 fused_linear: bool = False,
                 sampler: Optional["DeviceSampler"] = None):
        _check_fused_linear(fused, fused_linear)
        dev = next(model.parameters()).device
        batch = cache.attn_prev[0].shape[0]
        self.seq_len = model.cfg.seq_len
        if not 0 <= start_pos < self.seq_len:
            raise IndexError(f"decode start position {start_pos} outside "
                             f"[0, {self.seq_len})")
        # host mirror of pos_dev: step() refuses a replay past seq_len
        # before it is launched (the kernels' own position guard is the
        # second line of defence)
        self.next_pos = start_pos
        self.fused = fused
        self.fused_linear = fused_linear
        if fused:
            def step_fn(model, token, cache, pos_dev):
                return forward_step_fused(model, token, cache, pos_dev,
                                          fused_linear=fused_linear)
        else:
            step_fn = forward_step_static
        self.cache = cache
        self.sampler = sampler
        self.token = torch.zeros(batch, dtype=torch.long, device=dev)
        self.pos_dev = torch.tensor(start_pos, dtype=torch.long, device=dev)
        if sampler is not None:
            forward_fn = step_fn

            def step_fn(model, token, cache, pos_dev):
                logits = forward_fn(model, token, cache, pos_dev)
                sampler.sample(logits, pos_dev, token)
                return logits

        # warmup + capture perturb the cache and pos — and, with a sampler,
        # seq, pads and the token buffer; snapshot & restore
        sampled = [] if sampler is None else \
            [sampler.seq, sampler.pads, self.token]
        snap = {
            "sampled": [t.clone() for t in sampled],
            "k": [t.clone() for t in cache.k],
            "v": [t.clone() for t in cache.v],
            "ap": [t.clone() for t in cache.attn_prev],
            "fp": [t.clone() for t in cache.ff_prev],
            "gh": [t.clone() for t in cache.gate_hist if t is not None],
            "pos": self.pos_dev.clone(),
        }

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            # every warmup step runs AT start_pos (the cache is restored
            # below), so warming up never indexes past seq_len
            for _ in range(warmup):
                step_fn(model, self.token, cache, self.pos_dev)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()

        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.static_logits = step_fn(
                model, self.token, cache, self.pos_dev)
            self.pos_dev += 1  # in-graph position advance

        with torch.no_grad():
            for dst, src in zip(cache.k, snap["k"]):
                dst.copy_(src)
            for dst, src in zip(cache.v, snap["v"]):
                dst.copy_(src)
            for dst, src in zip(cache.attn_prev, snap["ap"]):
                dst.copy_(src)
            for dst, src in zip(cache.ff_prev, snap["fp"]):
                dst.copy_(src)
            gh = [t for t in cache.gate_hist if t is not None]
            for dst, src in zip(gh, snap["gh"]):
                dst.copy_(src)
            for dst, src in zip(sampled, snap["sampled"]):
                dst.copy_(src)
            self.pos_dev.copy_(snap["pos"])
        torch.cuda.synchronize()

    def step(self, tokens: torch.Tensor) -> torch.Tensor:
        """Replay one decode step. ``tokens``: (B,) int64 (host or
        device); returns the (B, V) static logits tensor — copy it out
        before the next replay. Raises IndexError, without replaying,
        once the position has reached seq_len."""
        if self.next_pos >= self.seq_len:
            raise IndexError(f"decode past seq_len ({self.seq_len})")
        self.token.copy_(tokens.reshape(-1), non_blocking=False)
        self.graph.replay()
        self.next_pos += 1
        self.cache.pos = self.next_pos
        return self.static_logits

    def replay(self, n: int = 1) -> None:
        """Replay ``n`` self-feeding steps back to back (needs a
        ``sampler``): each reads the token the one before it sampled. No
        host synchronisation and no copy in between. Raises IndexError,
        without replaying, if that would pass seq_len."""
        if self.sampler is None:
            raise RuntimeError("replay() needs a GraphedDecodeStep built "
                               "with a sampler; use step(tokens)")
        if n < 0 or self.next_pos + n > self.seq_len:
            raise IndexError(f"decode past seq_len ({self.seq_len})")
        for _ in range(n):
            self.graph.replay()
        self.next_pos += n
        self.cache.pos = self.next_pos


def _check_fused_linear(fused: bool, fused_linear: bool) -> None:
    if fused_linear and not fused:
        raise ValueError("fused_linear=True needs fused=True: the decode "
                         "linear kernel is part of the fused decode step")


def _eager_step(model: ProGenBase, token: torch.Tensor, cache: DecodeCache,
                pos_dev: Optional[torch.Tensor],
                fused_linear: bool = False) -> torch.Tensor:
    """One uncaptured decode step that advances the cache position.
    ``pos_dev`` None: ``forward_step``; else ``forward_step_fused`` at the
    device position ``pos_dev``, which is kept equal to ``cache.pos``."""
    if pos_dev is None:
        return forward_step(model, token, cache)
    if cache.pos >= model.cfg.seq_len:
        raise IndexError(f"decode past seq_len ({model.cfg.seq_len})")
    logits = forward_step_fused(model, token, cache, pos_dev,
                                fused_linear=fused_linear)
    pos_dev += 1
    cache.pos += 1
    return logits


def _sample_batch_on_device(model: ProGenBase, seq: torch.Tensor, lens,
                            top_k: Optional[int], seed: Optional[int], dev,
                            graph: bool, fused: bool, fused_linear: bool,
                            check_every: int,
                            prefill: bool = False) -> torch.Tensor:
    """``sample_cached_batch`` with the sampler on the device: every step is
    forward + ``OF.decode_sample`` + position increment, and the host only
    looks at the pad counts every ``check_every`` steps. ``seq`` (B, length)
    holds the primes, ``lens`` their lengths. ``prefill``: as in
    ``sample_cached_batch``."""
    if check_every < 1:
        raise ValueError(f"check_every must be >= 1, got {check_every}")
    dev = torch.device(dev)
    B, length = seq.shape
    if top_k is not None and seed is None:
        # the host path would draw its noise from the global generator
        seed = int(torch.randint(0, 2 ** 63 - 1, (1,)))
    cache = DecodeCache(model, batch=B, device=dev)
    start = _prefill_common_prefix(model, seq, lens, cache) if prefill else 0
    sampler = DeviceSampler(seq, lens, top_k, seed, dev, written=start + 1)
    steps = length - 1 - start
    done = 0
    if graph and dev.type == "cuda":
        graphed = GraphedDecodeStep(model, cache, start_pos=start,
                                    fused=fused, fused_linear=fused_linear,
                                    sampler=sampler)
        # H2D memcpy, no kernel
        graphed.token.copy_(seq[:, start].contiguous())

        def run(n):
            graphed.replay(n)
    else:
        token = seq[:, start].contiguous().to(dev, copy=True)
        pos_dev = torch.full((), start, dtype=torch.long).to(dev)

        def run(n):
            for _ in range(n):
                if fused:
                    # advances pos_dev itself, after the forward: sample
                    # at the position the step ran at
                    if cache.pos >= model.cfg.seq_len:
                        raise IndexError(
                            f"decode past seq_len ({model.cfg.seq_len})")
                    logits = forward_step_fused(model, token, cache, pos_dev,
                                                fused_linear=fused_linear)
                    cache.pos += 1
                else:
                    # forward_step keeps its position on the host; the
                    # sampler needs a device position of its own
                    logits = forward_step(model, token, cache)
                sampler.sample(logits, pos_dev, token)
                pos_dev.add_(1)

    while done < steps:
        n = min(check_every, steps - done)
        run(n)
        done += n
        if bool((sampler.pads.cpu() >= 2).all()):
            break  # every row has emitted its EOS

    out = sampler.seq.cpu()
    remove_after_eos = (out == 0).long().cumsum(dim=-1) > 1
    return out * (~remove_after_eos).long()


@torch.no_grad()
def sample_cached(
    model: ProGenBase,
    prime: torch.Tensor,
    length: int,
    top_k: Optional[int] = None,
    add_bos: bool = False,
    generator: Optional[torch.Generator] = None,
    device=None,
    graph: bool = False,
    fused: bool = False,
    fused_linear: bool = False,
    device_sampling: bool = False,
    seed: Optional[int] = None,
    check_every: int = 16,
    prefill: bool = False,
) -> torch.Tensor:
    """Drop-in ``utils.sample`` with O(window + n_sgu) per-token cost.

    Same decoding semantics (reference: utils.py:106-135): gumbel-max with
    strict-> top-k masking (excluded logits -> 0, not -inf), pad-to-length
    output, everything after the second pad/EOS zeroed. Stops forwarding
    at EOS instead of emitting to full length.

    ``fused=True`` runs prefill and decode on ``forward_step_fused`` (the
    decode kernels on a GPU); combinable with ``graph``.
    ``fused_linear=True`` (needs ``fused``) also runs its projections on
    the decode linear kernel.

    ``device_sampling=True`` is row 0 of ``sample_cached_batch`` with the
    same flag, ``seed`` and ``check_every`` (see there); ``add_bos``
    prepends a 0 to the prime.

    ``prefill=True`` builds the cache of the prime with one forward over
    all its tokens (``prefill``) instead of one decode step per token,
    where ``prefill_supported``; elsewhere it changes nothing."""
    _check_fused_linear(fused, fused_linear)
    if device_sampling:
        prime = torch.as_tensor(prime).long().flatten().cpu()
        if add_bos:
            prime = F.pad(prime, (1, 0))
        return sample_cached_batch(
            model, [prime], length, top_k=top_k, generator=generator,
            device=device, graph=graph, fused=fused,
            fused_linear=fused_linear, device_sampling=True, seed=seed,
            check_every=check_every, prefill=prefill)[0]
    if seed is not None:
        raise ValueError("seed= keys the device sampler; without "
                         "device_sampling=True pass generator=")
    dev = next(model.parameters()).device if device is None else device
    # the sequence and sampling math live on CPU (matching utils.sample's
    # generator semantics — its fn closure returns .cpu() logits); only
    # the forward_step runs on the model device
    prime = torch.as_tensor(prime).long().flatten().cpu()
    start_pos = prime.shape[-1]
    pad = (0, length - start_pos) if not add_bos else (1, length - start_pos - 1)
    seq = F.pad(prime, pad)
    if add_bos:
        start_pos += 1

    cache = DecodeCache(model, batch=1, device=dev)
    pos_dev = torch.zeros((), dtype=torch.long, device=dev) if fused else None
    logits = None
    done = False
    if prefill:
        done, logits = _prefill_if_supported(
            model, seq[:start_pos].unsqueeze(0), cache, pos_dev, True)
    for p in range(0 if done else start_pos):            # prefill by steps
        logits = _eager_step(model, seq[p:p + 1].to(dev), cache, pos_dev,
                             fused_linear)

    graphed = None
    if graph and dev.type == "cuda":
        logits = logits.clone()  # the static buffer will be reused
        graphed = GraphedDecodeStep(model, cache, start_pos=start_pos,
                                    fused=fused, fused_linear=fused_linear)

    pads_seen = int((seq[:start_pos] == 0).sum())
    for curr_pos in range(start_pos, length):
        logits_row = logits[0].cpu().float()  # D2H then host cast: no device kernel between replays
        noise = R.gumbel_noise(logits_row.shape, generator=generator,
                               device=logits_row.device)
        if top_k is not None:
            mask, logits_row = R.select_top_k(logits_row, top_k)
            noise = noise * mask
        sampled = (logits_row + noise).argmax(dim=-1)
        seq[curr_pos] = sampled
        if sampled.item() == 0:
            pads_seen += 1
            if pads_seen >= 2:
                break
        if curr_pos + 1 < length:
            if graphed is not None:
                logits = graphed.step(seq[curr_pos:curr_pos + 1])
            else:
                logits = _eager_step(model,
                                     seq[curr_pos:curr_pos + 1].to(dev),
                                     cache, pos_dev, fused_linear)

    remove_after_eos = (seq == 0).long().cumsum(dim=-1) > 1
    return seq * (~remove_after_eos).long()


@torch.no_grad()
def sample_cached_batch(
    model: ProGenBase,
    primes,
    length: int,
    top_k: Optional[int] = None,
    generator: Optional[torch.Generator] = None,
    device=None,
    graph: bool = False,
    fused: bool = False,
    fused_linear: bool = False,
    device_sampling: bool = False,
    seed: Optional[int] = None,
    check_every: int = 16,
    prefill: bool = False,
) -> torch.Tensor:
    """Batched incremental decode: one forward_step advances ALL rows
    (the per-layer caches are batch-first), so serving throughput scales
    with batch at the same per-step latency.

    ``primes``: list of 1-D int tensors (ragged). Shorter primes are
    left-padded into the batch by decoding their sampled continuations
    only after their own prime ends — implemented by overwriting
    positions < len(prime_i) with the prime tokens. Rows that hit their
    second pad/EOS keep emitting into a dead tail that is zeroed at the
    end (same zero-after-second-pad rule as ``utils.sample``). With
    ``top_k=None`` and ``generator=None`` decoding is greedy argmax and
    each row's output equals its single-row ``sample_cached`` run
    (tests/test_decode.py::test_sample_cached_batch_greedy_parity).
    ``fused=True`` steps with ``forward_step_fused``; combinable with
    ``graph``. ``fused_linear=True`` (needs ``fused``) also runs its
    projections on the decode linear kernel.

    ``device_sampling=True`` keeps the sequences, the pad counts and the
    token on the device and samples there (``OF.decode_sample``: the HIP
    kernel on a GPU, inside the captured step with ``graph``; the reference
    on the CPU). The host neither downloads logits nor uploads tokens: it
    downloads the pad counts after every ``check_every`` steps to see
    whether every row has finished, and the sequences once at the end.
    Tokens emitted past a row's second pad are zeroed by the final rule, so
    the result does not depend on ``check_every``. ``seed`` (an int in
    [0, 2^63)) keys the sampler's Philox stream, which is its own and not
    torch's: ``generator`` is refused. ``top_k=None`` with ``seed=None`` is
    greedy and equals the host path's greedy output; ``top_k`` without a
    seed draws one from torch's global generator on the host.

    ``prefill=True`` builds the cache of the primes' common prefix, their
    first min(len) - 1 positions, with one forward (``prefill``) where
    ``prefill_supported``, and steps on from there; the tokens are those
    of the step loop up to fp reduction order."""
    _check_fused_linear(fused, fused_linear)
    dev = next(model.parameters()).device if device is None else device
    primes = [torch.as_tensor(p).long().flatten().cpu() for p in primes]
    B = len(primes)
    lens = [int(p.shape[-1]) for p in primes]
    seq = torch.zeros(B, length, dtype=torch.long)
    for i, p in enumerate(primes):
        seq[i, :lens[i]] = p
    if device_sampling:
        if generator is not None:
            raise ValueError(
                "device_sampling=True draws from the sampler's own Philox "
                "stream, keyed by seed=; generator= cannot drive it")
        return _sample_batch_on_device(model, seq, lens, top_k, seed, dev,
                                       graph, fused, fused_linear,
                                       check_every, prefill)
    if seed is not None:
        raise ValueError("seed= keys the device sampler; without "
                         "device_sampling=True pass generator=")

    cache = DecodeCache(model, batch=B, device=dev)
    start = _prefill_common_prefix(model, seq, lens, cache) if prefill else 0
    graphed = GraphedDecodeStep(model, cache, start_pos=start, fused=fused,
                                fused_linear=fused_linear) \
        if (graph and dev.type == "cuda") else None
    # the graphed step owns its device position; the eager fused one needs one
    pos_dev = torch.full((), start, dtype=torch.long, device=dev) \
        if (fused and graphed is None) else None
    greedy = top_k is None and generator is None
    # per-row pad counts over WRITTEN tokens only (the unfilled zero tail
    # must not count as EOS); positions 0..start are written at entry
    pads = [int((seq[i, :start + 1] == 0).sum()) for i in range(B)]
    for pos in range(start, length - 1):
        if graphed is not None:
            logits = graphed.step(seq[:, pos])
        else:
            logits = _eager_step(model, seq[:, pos].to(dev), cache,
                                 pos_dev, fused_linear)  # (B, V)
        rows = logits.cpu().float()  # no device kernel between replays
        if greedy:
            nxt = rows.argmax(dim=-1)
        else:
            noise = R.gumbel_noise(rows.shape, generator=generator)
            if top_k is not None:
                mask, rows = R.select_top_k(rows, top_k)
                noise = noise * mask
            nxt = (rows + noise).argmax(dim=-1)
        w = pos + 1
        # keep prime tokens where the prime extends past this position
        for i in range(B):
            if w >= lens[i]:
                seq[i, w] = nxt[i]
            pads[i] += int(seq[i, w] == 0)
        if all(p >= 2 for p in pads):
            break  # every row has emitted its EOS

    remove_after_eos = (seq == 0).long().cumsum(dim=-1) > 1
    return seq * (~remove_after_eos).long()
