"""Pure-PyTorch reference implementations of every ProGen op.

These serve two purposes:
  1. the CPU execution path (this container has no GPU), and
  2. the fp32 numerics oracle that every hand-written HIP kernel is
     tested against (tests/test_ops.py, tests/test_gpu_kernels.py).

Semantics mirror the JAX reference exactly, including its quirks:
  - GPT-J interleaved rotary applied to q, k AND v
    (reference: progen_transformer/progen.py:24-41,87)
  - token shift of the first ceil(d/2) channels by +1 position
    (reference: progen.py:43-46)
  - scale-only LayerNorm, no offset (reference: progen.py:22)
  - local window attention with one-window lookback where window 0's
    lookback keys are all-zero and UNMASKED (reference: progen.py:88-96)
  - masked cross-entropy where the first pad token is learned as EOS
    (reference: progen_transformer/utils.py:45-59)

All functions are batch-first: x is (B, N, ...) unlike the reference's
unbatched (N, ...) traced-through-vmap layout.
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn.functional as F

ATTN_MASK_VALUE = -1e10  # reference: progen.py:18


# ---------------------------------------------------------------------------
# rotary embedding (GPT-J interleaved)
# ---------------------------------------------------------------------------

def fixed_pos_embedding(
    seq: int, dim: int, dtype: torch.dtype = torch.float32,
    device: Optional[torch.device] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """sin/cos tables of shape (seq, dim).

    Each frequency is repeated twice along the last axis, i.e. elements
    2i and 2i+1 share inv_freq[i]  (reference: progen.py:24-28 — the
    ``repeat 'b n -> b (n r)', r=2``).
    """
    inv_freq = 1.0 / (
        10000 ** (torch.arange(0, dim, 2, dtype=torch.float64, device=device) / dim)
    )
    t = torch.arange(seq, dtype=torch.float64, device=device)
    sinusoid = torch.einsum("i,j->ij", t, inv_freq)           # (seq, dim/2)
    sinusoid = sinusoid.repeat_interleave(2, dim=-1)          # (seq, dim)
    return sinusoid.sin().to(dtype), sinusoid.cos().to(dtype)


def rotate_every_two(x: torch.Tensor) -> torch.Tensor:
    """(x0, x1, x2, x3, ...) -> (-x1, x0, -x3, x2, ...)  (reference: progen.py:30-34)."""
    x1 = x[..., 0::2]
    x2 = x[..., 1::2]
    return torch.stack((-x2, x1), dim=-1).flatten(-2)


def apply_rotary_pos_emb(
    x: torch.Tensor, sin: torch.Tensor, cos: torch.Tensor
) -> torch.Tensor:
    """Apply interleaved rotary over the FULL last dim (rot_dim == dim_head in
    the reference, progen.py:36-41). x: (..., n, d); sin/cos: (n, d)."""
    return x * cos + rotate_every_two(x) * sin


# ---------------------------------------------------------------------------
# token shift
# ---------------------------------------------------------------------------

def shift_tokens(x: torch.Tensor) -> torch.Tensor:
    """Shift the first ceil(d/2) channels by +1 position (pad front, drop
    last). x: (B, N, D).  (reference: progen.py:43-46; np.array_split puts
    the extra channel in the FIRST half for odd D.)"""
    d = x.shape[-1]
    split = -(-d // 2)  # ceil — matches np.array_split(x, 2, axis=-1)
    x_shift, x_pass = x[..., :split], x[..., split:]
    x_shift = F.pad(x_shift, (0, 0, 1, 0))[:, :-1]
    return torch.cat((x_shift, x_pass), dim=-1)


# ---------------------------------------------------------------------------
# scale-only LayerNorm (+ optional fused token shift)
# ---------------------------------------------------------------------------

def layernorm_nobias(
    x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5
) -> torch.Tensor:
    """LayerNorm with learned scale, no offset (reference: progen.py:22 —
    hk.LayerNorm(create_scale=True, create_offset=False, axis=-1)).

    Statistics are computed in fp32 regardless of input dtype."""
    orig_dtype = x.dtype
    if x.dtype in (torch.bfloat16, torch.float16):
        x = x.float()
    mu = x.mean(dim=-1, keepdim=True)
    var = x.var(dim=-1, unbiased=False, keepdim=True)
    y = (x - mu) * torch.rsqrt(var + eps)
    return (y * weight.to(y.dtype)).to(orig_dtype)


def ln_shift(
    x: torch.Tensor, weight: torch.Tensor, shift: bool = True, eps: float = 1e-5
) -> torch.Tensor:
    """Fused LN -> token-shift prologue used by both branches
    (reference: progen.py:74-77 and progen.py:132-135)."""
    y = layernorm_nobias(x, weight, eps)
    if shift:
        y = shift_tokens(y)
    return y


# ---------------------------------------------------------------------------
# local window attention core
# ---------------------------------------------------------------------------

def local_attention(
    qkv: torch.Tensor,
    sin: torch.Tensor,
    cos: torch.Tensor,
    heads: int,
    window_size: int,
) -> torch.Tensor:
    """Windowed causal attention with one-window lookback.

    qkv: (B, N, 3*h*dh) — output of the bias-free QKV projection
         (reference: progen.py:70,83).
    sin/cos: (N, dh) rotary tables.
    Returns (B, N, h*dh) in the merged '(w n) (h d)' layout
    (reference: progen.py:85-102).

    Quirks preserved:
      - rotary is applied to q, k AND v (reference: progen.py:87)
      - window 0's lookback keys are the zero-pad window and are NOT
        masked: their logit is exactly 0 pre-scale and enters the softmax
        denominator (reference: progen.py:90-96)
      - mask = tril(ones(wsz, 2*wsz), k=wsz): full previous window plus
        causal own window (reference: progen.py:95)
      - pre-softmax max-subtraction with stop_gradient (progen.py:98)
    """
    B, N, three_inner = qkv.shape
    dh = three_inner // (3 * heads)
    wsz = window_size
    assert N % wsz == 0, "sequence length must be divisible by the window size"
    w = N // wsz
    scale = dh ** -0.5

    q, k, v = qkv.chunk(3, dim=-1)
    # (B, N, h*dh) -> (B, h, N, dh)
    def to_heads(t: torch.Tensor) -> torch.Tensor:
        return t.view(B, N, heads, dh).transpose(1, 2)

    q, k, v = map(to_heads, (q, k, v))

    sin = sin.to(q.dtype)
    cos = cos.to(q.dtype)
    q, k, v = (apply_rotary_pos_emb(t, sin, cos) for t in (q, k, v))

    # window: (B, h, w, wsz, dh)
    q = q.view(B, heads, w, wsz, dh)
    k = k.view(B, heads, w, wsz, dh)
    v = v.view(B, heads, w, wsz, dh)

    # one-window lookback: pad a zero window in front, build [prev ‖ own]
    # (reference: progen.py:90-91)
    k = F.pad(k, (0, 0, 0, 0, 1, 0))
    v = F.pad(v, (0, 0, 0, 0, 1, 0))
    k = torch.cat((k[:, :, :-1], k[:, :, 1:]), dim=3)   # (B, h, w, 2*wsz, dh)
    v = torch.cat((v[:, :, :-1], v[:, :, 1:]), dim=3)

    sim = torch.einsum("bhwid,bhwjd->bhwij", q, k) * scale

    mask = torch.ones(wsz, 2 * wsz, dtype=torch.bool, device=qkv.device).tril(wsz)
    # masked_fill with a python scalar (not torch.tensor(...): that is an
    # H2D op, illegal under hipGraph capture — needed by the
    # PROGEN_FORCE_EAGER-in-graph bisect path of the replay investigation)
    sim = sim.masked_fill(~mask, ATTN_MASK_VALUE)

    sim = sim - sim.amax(dim=-1, keepdim=True).detach()
    attn = sim.softmax(dim=-1)

    out = torch.einsum("bhwij,bhwjd->bhwid", attn, v)
    # 'h w n d -> (w n) (h d)'
    out = out.permute(0, 2, 3, 1, 4).reshape(B, N, heads * dh)
    return out


# ---------------------------------------------------------------------------
# GLU feedforward epilogue
# ---------------------------------------------------------------------------

def glu_gelu(x: torch.Tensor) -> torch.Tensor:
    """x, gate = split(h, 2); x * gelu(gate)  (reference: progen.py:139-141).

    The reference's jax.nn.gelu is the tanh approximation (JAX default
    approximate=True); we use the same."""
    x, gate = x.chunk(2, dim=-1)
    return x * F.gelu(gate, approximate="tanh")


def gelu(x: torch.Tensor) -> torch.Tensor:
    """Plain GELU branch for non-GLU FF (reference: progen.py:143)."""
    return F.gelu(x, approximate="tanh")


# ---------------------------------------------------------------------------
# SGU — gMLP spatial gating unit
# ---------------------------------------------------------------------------

def sgu_gate(
    x: torch.Tensor,
    norm_weight: torch.Tensor,
    spatial_weights: torch.Tensor,
    spatial_biases: torch.Tensor,
    eps: float = 1e-5,
) -> torch.Tensor:
    """Spatial gating: split hidden in half, LN the gate half, apply the
    causal learned (n, n) spatial matrix, multiply
    (reference: progen.py:166-183).

    x: (B, N, H) with H even; returns (B, N, H/2) — the gated half
    BEFORE the output projection (proj_out is a plain GEMM, done by the
    caller)."""
    xa, gate = x.chunk(2, dim=-1)
    gate = layernorm_nobias(gate, norm_weight, eps)

    n = x.shape[1]
    w = spatial_weights[:n, :n].tril()  # mask = tril(ones(n, n)) (progen.py:179-180)
    # gate_out[m, d] = sum_n W[m, n] * gate[n, d] + b[m]
    gate = torch.einsum("bnd,mn->bmd", gate, w.to(gate.dtype)) + spatial_biases[:n].to(gate.dtype)
    return xa * gate


# ---------------------------------------------------------------------------
# masked cross-entropy with first-pad-as-EOS
# ---------------------------------------------------------------------------

def masked_mean(t: torch.Tensor, mask: torch.Tensor, dim=None) -> torch.Tensor:
    """(reference: utils.py:42-43)"""
    mask = mask.to(t.dtype)
    return (t * mask).sum(dim=dim) / mask.sum(dim=dim)


def cross_entropy(
    logits: torch.Tensor, targets: torch.Tensor, ignore_index: int = 0
) -> torch.Tensor:
    """Per-sequence masked CE, then mean over batch.

    mask = (targets != 0) extended by the first pad position, so the model
    learns the first pad as EOS (reference: utils.py:45-59). The reference
    computes a per-sequence masked mean inside vmap and then a plain mean
    over the batch (utils.py:67,75-76) — we preserve that exact reduction
    order (NOT a global masked mean).

    logits: (B, N, V); targets: (B, N) int64. Softmax in fp32.
    """
    if logits.dtype in (torch.bfloat16, torch.float16):
        logits = logits.float()  # softmax statistics in >= fp32
    logprobs = F.log_softmax(logits, dim=-1)
    nll = logprobs.gather(-1, targets.unsqueeze(-1).long()).squeeze(-1)

    mask = targets != ignore_index
    eos_mask = (~mask).long().cumsum(dim=-1) == 1
    mask = mask | eos_mask

    ce_per_seq = -masked_mean(nll, mask, dim=-1)  # (B,)
    return ce_per_seq.mean()


# ---------------------------------------------------------------------------
# sampling helpers
# ---------------------------------------------------------------------------

def select_top_k(t: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-k mask with the reference's quirks: strict `>` against the k-th
    value (may select fewer than k on ties) and excluded logits set to 0,
    not -inf (reference: utils.py:97-100)."""
    values, _ = t.topk(k, dim=-1)
    mask = t > values.amin(dim=-1, keepdim=True)
    return mask, torch.where(mask, t, torch.zeros_like(t))


def gumbel_noise(shape, generator=None, device=None, dtype=torch.float32) -> torch.Tensor:
    u = torch.rand(shape, generator=generator, device=device, dtype=dtype)
    eps = 1e-20  # reference: utils.py:20-21 log(t + eps)
    return -torch.log(-torch.log(u + eps) + eps)


# ---------------------------------------------------------------------------
# fused decode-step ops (one row per batch element; ops/hip/decode_*.hip)
# ---------------------------------------------------------------------------
# Same signatures and in-place cache effects as the kernels. Tensor indexing
# only: ``pos`` is a 0-dim int64 tensor and no shape depends on its value,
# so a step built from these is position-static (decode.forward_step_static).
# Cache rows a step must not read are dropped with ``where``, never
# multiplied by zero, so whatever they hold cannot leak into the result.

def decode_ln_shift(
    h: torch.Tensor,
    res: Optional[torch.Tensor],
    g: torch.Tensor,
    prev: Optional[torch.Tensor],
    shift: bool,
    eps: float = 1e-5,
) -> torch.Tensor:
    """Residual add + scale-only LN + token shift on (B, D) rows.

    ``h`` becomes h + res in place (rounded to its dtype; the LN reads it
    as stored). Returns y = [prev[:, :split] | ln[:, split:]] when ``shift``
    else ln, then ``prev`` becomes ln. ``prev=None`` needs shift=False."""
    if res is not None:
        h.add_(res)
    ln = layernorm_nobias(h, g, eps)
    if shift:
        assert prev is not None, "shift needs the previous row"
        split = -(-h.shape[-1] // 2)
        y = torch.cat((prev[:, :split], ln[:, split:]), dim=-1)
    else:
        y = ln
    if prev is not None:
        prev.copy_(ln)
    return y


def decode_attention(
    qkv: torch.Tensor,
    rsin: torch.Tensor,
    rcos: torch.Tensor,
    pos: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    window: int,
) -> torch.Tensor:
    """One local-attention row at position ``pos``.

    qkv: (B, 3*H*dh) unrotated; k_cache/v_cache: (B, H, N, dh), row ``pos``
    is written with the rotated k and v. Attends over cache rows
    [max(0, w0 - window), pos], w0 = (pos // window) * window; while
    pos < window the ``window`` all-zero lookback keys of the full forward
    enter the softmax unmasked (logit 0, value 0). Returns (B, H*dh)."""
    B, H, N, dh = k_cache.shape
    p = pos.reshape(1)
    sc = rcos.index_select(0, p)[0].to(qkv.dtype)
    ss = rsin.index_select(0, p)[0].to(qkv.dtype)
    q, k, v = qkv.view(B, 3, H, dh).unbind(1)
    q, k, v = (t * sc + rotate_every_two(t) * ss for t in (q, k, v))
    k_cache.index_copy_(2, p, k.unsqueeze(2))
    v_cache.index_copy_(2, p, v.unsqueeze(2))

    # fixed 2*window band starting one window before the current one
    idx = (pos // window) * window - window + \
        torch.arange(2 * window, device=qkv.device)
    halo = idx < 0                  # zero lookback keys: logit 0, unmasked
    live = (idx >= 0) & (idx <= pos)
    safe = idx.clamp(min=0)
    zero = torch.zeros((), dtype=qkv.dtype, device=qkv.device)
    keys = torch.where(live.view(1, 1, -1, 1),
                       k_cache.index_select(2, safe), zero)
    vals = torch.where(live.view(1, 1, -1, 1),
                       v_cache.index_select(2, safe), zero)
    s = torch.einsum("bhd,bhnd->bhn", q, keys) * (dh ** -0.5)
    s = s.masked_fill(~(live | halo).view(1, 1, -1), -1e30)
    s = s - s.amax(dim=-1, keepdim=True)
    # softmax in fp32 for the 16-bit dtypes; fp32 and fp64 keep their own
    if s.dtype in (torch.bfloat16, torch.float16):
        a = s.float().softmax(dim=-1).to(qkv.dtype)
    else:
        a = s.softmax(dim=-1)
    return torch.einsum("bhn,bhnd->bhd", a, vals).reshape(B, H * dh)


def decode_sgu(
    h: torch.Tensor,
    g: torch.Tensor,
    hist: torch.Tensor,
    w: torch.Tensor,
    bias: torch.Tensor,
    pos: torch.Tensor,
    eps: float = 1e-5,
) -> torch.Tensor:
    """One spatial-gating row at position ``pos``.

    h: (B, 2*d2) = [xa | gate]; hist: (B, N, d2) LN'd gate rows, row ``pos``
    is written; w: (N, N); bias: (N, 1). Returns
    xa * (sum_{n <= pos} w[pos, n] * hist[:, n] + bias[pos]), (B, d2)."""
    p = pos.reshape(1)
    xa, gate = h.chunk(2, dim=-1)
    gl = layernorm_nobias(gate, g, eps)
    hist.index_copy_(1, p, gl.unsqueeze(1))
    n = hist.shape[1]
    past = torch.arange(n, device=h.device) <= pos
    zero = torch.zeros((), dtype=hist.dtype, device=h.device)
    rows = torch.where(past.view(1, -1, 1), hist, zero)
    w_row = w.index_select(0, p)[0, :n].to(hist.dtype)
    gate_out = torch.einsum("n,bnd->bd", w_row, rows) + \
        bias.index_select(0, p)[0].to(hist.dtype)
    return xa * gate_out


def decode_linear(x: torch.Tensor, w: torch.Tensor, bias, act: str = "none"
                  ) -> torch.Tensor:
    """``F.linear`` followed by the activation, in the input dtype: what the
    decode step computes with separate ops. ``act``: "none", "gelu" or
    "glu" (the output is then half as wide, ``glu_gelu``'s pairing)."""
    h = F.linear(x, w, bias)
    if act == "glu":
        return glu_gelu(h)
    if act == "gelu":
        return gelu(h)
    if act != "none":
        raise ValueError(f"decode_linear: unknown act {act!r}")
    return h


# ---------------------------------------------------------------------------
# prefill of the decode caches (ops/hip/prefill.hip)
# ---------------------------------------------------------------------------
# One full-sequence forward over the prime leaves in the caches what the
# decode steps of its positions would have stored. ``P`` is a host int; only
# cache rows [0, P) are written. Everything runs in the inputs' dtype.
#
# With ``admit``, a (B, 2) int64 tensor of [slot, rows] per batch row, the
# caches have any number S of rows: batch row b fills rows [0, min(rows, P))
# of cache row ``slot`` when 0 <= slot < S, and no cache row otherwise
# (ops/hip/prefill_admit.hip). The values are read on the host here, so like
# the slot references these cannot be captured in a graph.

def _admitted(admit: torch.Tensor, B: int, S: int, P: int):
    """(batch row, slot, rows) of every batch row of ``admit`` that stores
    anything."""
    assert admit.dtype == torch.int64 and admit.shape == (B, 2), \
        f"admit must be int64 ({B}, 2), got {admit.dtype} {tuple(admit.shape)}"
    return [(b, slot, min(rows, P))
            for b, (slot, rows) in enumerate(admit.tolist())
            if 0 <= slot < S and rows > 0]


def prefill_rope_kv(
    qkv: torch.Tensor,
    rsin: torch.Tensor,
    rcos: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    P: int,
    admit: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Interleaved rotary on q, k and v of qkv (B, N, 3*H*dh) at positions
    0..N-1; the rotated k and v of rows < P are stored head-major into
    k_cache/v_cache (B, H, Nc, dh), or as ``admit`` says into (S, H, Nc, dh).
    Returns the rotated qkv."""
    B, N, C = qkv.shape
    S, H, Nc, dh = k_cache.shape
    if not 1 <= P <= min(N, Nc):
        raise ValueError(f"prefill_rope_kv: P must be in [1, {min(N, Nc)}], "
                         f"got {P}")
    x = qkv.reshape(B, N, 3 * H, dh)
    s = rsin[:N].to(qkv.dtype).reshape(1, N, 1, dh)
    c = rcos[:N].to(qkv.dtype).reshape(1, N, 1, dh)
    rot = x * c + rotate_every_two(x) * s
    if admit is None:
        k_cache[:, :, :P] = rot[:, :P, H:2 * H].transpose(1, 2)
        v_cache[:, :, :P] = rot[:, :P, 2 * H:].transpose(1, 2)
    else:
        for b, slot, n in _admitted(admit, B, S, P):
            k_cache[slot, :, :n] = rot[b, :n, H:2 * H].transpose(0, 1)
            v_cache[slot, :, :n] = rot[b, :n, 2 * H:].transpose(0, 1)
    return rot.reshape(B, N, C)


def prefill_attention(
    qkv: torch.Tensor,
    rsin: torch.Tensor,
    rcos: torch.Tensor,
    heads: int,
    window: int,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    P: int,
    admit: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """``local_attention`` over the whole (B, N, 3*H*dh) qkv, with the
    rotated k/v rows < P left in the caches (``admit``: in the rows of the
    slots it names)."""
    N = qkv.shape[1]
    prefill_rope_kv(qkv, rsin, rcos, k_cache, v_cache, P, admit)
    return local_attention(qkv, rsin[:N], rcos[:N], heads, window)


def prefill_gate_ln(
    x: torch.Tensor,
    g: torch.Tensor,
    hist: torch.Tensor,
    P: int,
    eps: float = 1e-5,
    admit: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Scale-only LN of the gate half of x (B, N, 2*d2); rows < P are stored
    into hist (B, Nc, d2), or as ``admit`` says into (S, Nc, d2). Returns the
    (B, N, d2) LN'd gate."""
    N, Nc = x.shape[1], hist.shape[1]
    if not 1 <= P <= min(N, Nc):
        raise ValueError(f"prefill_gate_ln: P must be in [1, {min(N, Nc)}], "
                         f"got {P}")
    gate_ln = layernorm_nobias(x.chunk(2, dim=-1)[1], g, eps)
    if admit is None:
        hist[:, :P] = gate_ln[:, :P]
    else:
        for b, slot, n in _admitted(admit, x.shape[0], hist.shape[0], P):
            hist[slot, :n] = gate_ln[b, :n]
    return gate_ln


def prefill_sgu(
    x: torch.Tensor,
    g: torch.Tensor,
    w: torch.Tensor,
    bias: torch.Tensor,
    hist: torch.Tensor,
    P: int,
    eps: float = 1e-5,
    admit: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """``sgu_gate`` over the whole (B, N, 2*d2) activation, with the LN'd
    gate rows < P left in ``hist`` (``admit``: in the rows of the slots it
    names)."""
    n = x.shape[1]
    gate_ln = prefill_gate_ln(x, g, hist, P, eps, admit)
    wl = w[:n, :n].tril().to(gate_ln.dtype)
    gate = torch.einsum("bnd,mn->bmd", gate_ln, wl) + \
        bias[:n].to(gate_ln.dtype)
    return x.chunk(2, dim=-1)[0] * gate


# ---------------------------------------------------------------------------
# decode-step sampler (ops/hip/decode_sample.hip)
# ---------------------------------------------------------------------------
# The device sampler draws its uniforms from Philox4x32-10, a stateless
# counter-based generator: a replayed graph needs no generator state. This
# stream is the sampler's own — it is NOT torch's generator stream.

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    """Philox4x32-10 on numpy arrays: ``counter`` (..., 4) and ``key``
    (..., 2) hold 32-bit words; returns the (..., 4) output words as uint64.
    Exact integer arithmetic: every product of two 32-bit words fits in
    uint64."""
    import numpy as np
    m32 = np.uint64(0xFFFFFFFF)
    c = [np.asarray(counter, dtype=np.uint64)[..., i] & m32 for i in range(4)]
    k = [np.asarray(key, dtype=np.uint64)[..., i] & m32 for i in range(2)]
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c[0]
        p1 = np.uint64(PHILOX_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & m32,
             (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & m32]
        k = [(k[0] + np.uint64(PHILOX_W0)) & m32,
             (k[1] + np.uint64(PHILOX_W1)) & m32]
    return np.stack(np.broadcast_arrays(*c), axis=-1)


def decode_sample_uniform(seed: int, w: int, B: int, V: int) -> torch.Tensor:
    """The sampler's uniforms for position ``w``: (B, V) fp32 in [0, 1).
    Key = (seed & 0xffffffff, seed >> 32), counter = (j, w, b, 0); output
    word i of block j belongs to vocabulary index 4j + i; u = (x >> 8) *
    2^-24, exact in fp32."""
    import numpy as np
    nblk = -(-V // 4)
    ctr = np.zeros((B, nblk, 4), dtype=np.uint64)
    ctr[..., 0] = np.arange(nblk, dtype=np.uint64)[None, :]
    ctr[..., 1] = np.uint64(w)
    ctr[..., 2] = np.arange(B, dtype=np.uint64)[:, None]
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF],
                   dtype=np.uint64)
    x = philox4x32_10(ctr, key).reshape(B, nblk * 4)[:, :V]
    u = (x >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return torch.from_numpy(u)


def decode_sample_scores(t: torch.Tensor, u: Optional[torch.Tensor],
                         top_k: int, greedy: bool) -> torch.Tensor:
    """The (B, V) fp32 scores whose first argmax is the sampled token.
    Greedy: the logits. Else t + g with g = -log(-log(u + 1e-20) + 1e-20)
    in fp32; with ``top_k`` > 0 only entries with fewer than ``top_k``
    entries >= them (select_top_k's strict > the k-th largest value) keep
    their score, every other entry scores exactly 0."""
    t = t.float()
    if greedy:
        return t
    eps = 1e-20
    g = -torch.log(-torch.log(u.float() + eps) + eps)
    if top_k <= 0:
        return t + g
    rank = (t.unsqueeze(1) >= t.unsqueeze(2)).sum(dim=-1)  # #{i: t_i >= t_j}
    sel = rank < top_k
    zero = torch.zeros_like(t)
    return torch.where(sel, t, zero) + torch.where(sel, g, zero)


def decode_sample(
    logits: torch.Tensor,
    pos: torch.Tensor,
    seed: torch.Tensor,
    seq: torch.Tensor,
    lens: torch.Tensor,
    pads: torch.Tensor,
    token: torch.Tensor,
    top_k: int = 0,
    greedy: bool = False,
    u_out: Optional[torch.Tensor] = None,
) -> None:
    """Sample position w = pos + 1 of every row, in place.

    logits (B, V); pos 0-dim int64; seed (1,) int64; seq (B, L), lens, pads
    and token (B,) int64. Row b's token is the first argmax of
    ``decode_sample_scores`` with the uniforms of ``decode_sample_uniform``;
    it is written to seq[b, w] unless the prime covers w (w < lens[b]); then
    pads[b] += (seq[b, w] == 0) and token[b] = seq[b, w]. ``u_out`` (B, V)
    fp32 receives the uniforms. With pos < 0 or w >= L nothing is touched.

    Goes through the host (the position and the seed are read there, and
    Philox runs in numpy), so it cannot be captured in a graph."""
    if logits.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError(
            "decode_sample: the reference sampler reads the position on the "
            "host and cannot be captured in a graph; capture needs the HIP "
            "kernel (do not list dec_sample in PROGEN_EAGER_OPS)")
    B, V = logits.shape
    L = seq.shape[1]
    p = int(pos)
    w = p + 1
    if p < 0 or w >= L:
        return
    u = None
    if not greedy:
        u = decode_sample_uniform(int(seed[0]), w, B, V)
        if u_out is not None:
            u_out.copy_(u)
    scores = decode_sample_scores(logits.detach().cpu(), u, int(top_k), greedy)
    sampled = scores.argmax(dim=-1).to(seq.device)  # first maximal index
    col = torch.where(lens <= w, sampled, seq[:, w])
    seq[:, w] = col
    pads.add_((col == 0).long())
    token.copy_(col)


# ---------------------------------------------------------------------------
# slot twins of the decode-step ops (progen_amd._C_decode_slots)
# ---------------------------------------------------------------------------
# One position per batch row: ``pos`` is (B,) int64 and pos[b] < 0 marks an
# idle row, which changes nothing and gets a zero output row. Each twin runs
# the scalar reference above on the row views b:b+1, so a row computes what
# it would compute alone at its position. The positions are read on the
# host: like ``decode_sample`` these cannot be captured in a graph.

def _slot_positions(pos: torch.Tensor, B: int, n: int):
    """(row, 0-dim position tensor) of every live row of a (B,) ``pos``;
    positions outside [0, n) are idle, as in the kernels."""
    assert pos.shape == (B,), f"pos must be ({B},), got {tuple(pos.shape)}"
    return [(b, pos[b]) for b, p in enumerate(pos.tolist()) if 0 <= p < n]


def decode_ln_shift_slots(
    h: torch.Tensor,
    res: Optional[torch.Tensor],
    g: torch.Tensor,
    prev: Optional[torch.Tensor],
    pos: torch.Tensor,
    shift: bool,
    eps: float = 1e-5,
) -> torch.Tensor:
    """``decode_ln_shift`` per row. A row at position 0 starts a request in a
    slot whose ``prev`` row belongs to the one before it: its shifted half is
    zeros. An idle row keeps its ``h`` and ``prev``."""
    y = torch.zeros_like(h)
    for b, p in enumerate(pos.tolist()):
        if p < 0:
            continue
        pb = None if prev is None else prev[b:b + 1]
        # at position 0 the shifted half is read from a zero stand-in; what
        # the scalar reference leaves in it (the LN row) goes to the real row
        rd = torch.zeros_like(pb) if p == 0 and pb is not None else pb
        y[b:b + 1] = decode_ln_shift(
            h[b:b + 1], None if res is None else res[b:b + 1], g, rd, shift,
            eps)
        if rd is not pb:
            pb.copy_(rd)
    return y


def decode_attention_slots(
    qkv: torch.Tensor,
    rsin: torch.Tensor,
    rcos: torch.Tensor,
    pos: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    window: int,
) -> torch.Tensor:
    """``decode_attention`` per row, row b at position pos[b]."""
    B, H, N, dh = k_cache.shape
    out = qkv.new_zeros(B, H * dh)
    for b, p in _slot_positions(pos, B, N):
        out[b:b + 1] = decode_attention(
            qkv[b:b + 1], rsin, rcos, p, k_cache[b:b + 1], v_cache[b:b + 1],
            window)
    return out


def decode_sgu_slots(
    h: torch.Tensor,
    g: torch.Tensor,
    hist: torch.Tensor,
    w: torch.Tensor,
    bias: torch.Tensor,
    pos: torch.Tensor,
    eps: float = 1e-5,
) -> torch.Tensor:
    """``decode_sgu`` per row, row b at position pos[b]."""
    B, N, d2 = hist.shape
    out = h.new_zeros(B, d2)
    for b, p in _slot_positions(pos, B, N):
        out[b:b + 1] = decode_sgu(h[b:b + 1], g, hist[b:b + 1], w, bias, p,
                                  eps)
    return out


def decode_sample_slots(
    logits: torch.Tensor,
    pos: torch.Tensor,
    token: torch.Tensor,
    seq: torch.Tensor,
    pads: torch.Tensor,
    ctl: torch.Tensor,
    u_out: Optional[torch.Tensor] = None,
) -> None:
    """``decode_sample`` with a position and a control row per batch row, in
    place; the sampler also owns the position advance and the retirement.

    logits (B, V); pos, token, pads (B,) and seq (B, L) int64; ctl (B, 5)
    int64 with columns [len, limit, top_k, seed, stream]. For row b with
    p = pos[b] >= 0 and w = p + 1: if w >= limit the row retires (pos[b] = -1)
    and nothing else changes. Else its token is the first argmax of
    ``decode_sample_scores``: greedy when seed < 0, else with ``top_k`` (0:
    the whole row) and row ``stream`` of the uniforms
    ``decode_sample_uniform(seed, w, stream + 1, V)``, i.e. the Philox counter
    (j / 4, w, stream, 0). It is written to seq[b, w] unless the prime covers
    w (w < len); then pads[b] += (seq[b, w] == 0), token[b] = seq[b, w] and
    pos[b] = -1 if pads[b] >= 2 or w + 1 >= limit, else w. ``u_out`` (B, V)
    fp32 receives the uniforms of the rows that drew any."""
    if logits.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError(
            "decode_sample_slots: the reference sampler reads the positions "
            "on the host and cannot be captured in a graph; capture needs the "
            "HIP kernel (do not list dec_sample in PROGEN_EAGER_OPS)")
    B, V = logits.shape
    L = seq.shape[1]
    rows = logits.detach().cpu()
    for b, p in enumerate(pos.tolist()):
        if p < 0:
            continue
        w = p + 1
        n, limit, top_k, seed, stream = ctl[b].tolist()
        if w >= limit or w >= L:
            pos[b] = -1
            continue
        greedy = seed < 0
        u = None
        if not greedy:
            u = decode_sample_uniform(seed, w, stream + 1, V)[stream:stream + 1]
            if u_out is not None:
                u_out[b:b + 1].copy_(u)
        scores = decode_sample_scores(rows[b:b + 1], u, top_k, greedy)
        tok = int(scores.argmax(dim=-1))  # first maximal index
        if w >= n:
            seq[b, w] = tok
        else:
            tok = int(seq[b, w])
        pads[b] += int(tok == 0)
        token[b] = tok
        pos[b] = -1 if (int(pads[b]) >= 2 or w + 1 >= limit) else w
