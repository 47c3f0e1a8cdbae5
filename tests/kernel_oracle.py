"""fp64 oracles, storage-precision emulations and the row-wise comparator
for the training kernels (tests/test_gpu_kernel_edges.py runs the kernels,
tests/test_kernel_oracle.py proves on the CPU that the comparator tells a
right kernel from a subtly wrong one). CPU only; nothing here needs a GPU.

Three computations of every op, on the rounded bf16/fp32 values a kernel
is handed:

  oracle     the functions of progen_amd/ops/reference.py in fp64 (autograd
             for the gradients), plus the per-row intermediates the kernels
             return (mean, rstd, nll, lse, gate_out, attention lse);
  emulation  the explicit forward/backward formulas (``*_explicit``) in
             fp32, rounded to bf16 exactly where the .hip source stores or
             stages bf16; for the fp32 instantiations nothing is rounded,
             i.e. the fp32 reference itself;
  mutants    the same explicit formulas with one deliberate defect.

The tolerance of a (family, dtype, output) is MARGIN x the emulation's
``row_err`` against the oracle, worst case over the family's cases
(``bounds``): what bf16 storage must cost, doubled for accumulation order
and the hardware exp/rsqrt, which the emulation does not model.
"""

from __future__ import annotations

import functools
import math

import torch
import torch.nn.functional as F

from progen_amd.ops import reference as R

BF16 = torch.bfloat16
F32 = torch.float32
F64 = torch.float64

MARGIN = 2.0
# a row quieter than 1/64 of the tensor's loudest element is measured
# against that 1/64: below it the absolute error of a bf16 sum of loud
# terms is all there is to see
FLOOR_FRAC = 2.0 ** -6


def ident(x):
    return x


def bf16_round(x):
    return x.to(BF16).to(x.dtype)


def rounder(dtype):
    return bf16_round if dtype == BF16 else ident


def dname(dtype) -> str:
    return {BF16: "bf16", F32: "fp32"}[dtype]


# ---------------------------------------------------------------------------
# comparator
# ---------------------------------------------------------------------------

def row_err(got, want, floor=None) -> float:
    """max over rows of max_d|got - want| / max(max_d|want|, floor), rows
    being the last dimension. ``floor`` defaults to FLOOR_FRAC of the
    loudest element of ``want``. Non-finite ``got`` is an infinite error."""
    got = got.detach().to("cpu", F64)
    want = want.detach().to("cpu", F64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not torch.isfinite(got).all():
        return math.inf
    if got.numel() == 0:
        return 0.0
    if got.dim() == 0:
        got, want = got.reshape(1, 1), want.reshape(1, 1)
    if floor is None:
        floor = FLOOR_FRAC * want.abs().max().item()
    floor = max(floor, 1e-300)
    diff = (got - want).abs().amax(dim=-1)
    scale = want.abs().amax(dim=-1).clamp_min(floor)
    return (diff / scale).max().item()


def elem_err(got, want, floor=None) -> float:
    """row_err with every element a row of its own: for the per-row scalars
    (mean, rstd, nll, lse) and flat optimizer state."""
    return row_err(got.reshape(-1, 1), want.reshape(-1, 1), floor)


def bf16_ordinal(x: torch.Tensor) -> torch.Tensor:
    """bf16 values as integers in value order (adjacent values differ by 1;
    +0 and -0 coincide)."""
    i = x.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def bf16_ulp_dist(got: torch.Tensor, want64: torch.Tensor) -> int:
    """largest distance, in bf16 steps, between ``got`` (bf16) and the
    correctly rounded ``want64``."""
    want = want64.detach().to("cpu", F64).to(BF16)
    got = got.detach().to("cpu")
    assert got.dtype == BF16 and got.shape == want.shape
    return int((bf16_ordinal(got) - bf16_ordinal(want)).abs().max().item())


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F32)


# ---------------------------------------------------------------------------
# ln_shift / ln_shift_res
# ---------------------------------------------------------------------------

def _ln_stats(s, eps, one_pass=False):
    mu = s.mean(-1, keepdim=True)
    if one_pass:
        var = ((s * s).mean(-1, keepdim=True) - mu * mu).clamp_min(0)
    else:
        var = ((s - mu) ** 2).mean(-1, keepdim=True)
    rs = torch.rsqrt(var + eps)
    return mu, rs


def _ln_bwd(e, g, xh, rs):
    """dx (before any ds) and dweight of y = xh * g for upstream ``e``."""
    eg = e * g
    a = (eg * xh).mean(-1, keepdim=True)
    b = eg.mean(-1, keepdim=True)
    dx = rs * (eg - b - xh * a)
    dw = (e * xh).reshape(-1, e.shape[-1]).sum(0)
    return dx, dw


def ln_explicit(x, res, g, dy, ds, shift, eps=1e-5, rnd=ident, mutant=None):
    """ln_shift.hip in formulas. Rounding points: s = x + res, y, dx, dw.
    The backward reads the saved fp32 statistics."""
    s = rnd(x + res) if res is not None else x
    B, N, D = s.shape
    half = D // 2
    mu, rs = _ln_stats(s, eps, one_pass=(mutant == "one_pass_var"))
    xh = (s - mu) * rs
    ln = rnd(xh * g)
    y, e = ln, dy
    if shift:
        if mutant == "shift_same_row":
            pass
        elif mutant == "shift_cross_batch":
            y = R.shift_tokens(ln.reshape(1, B * N, D)).reshape(B, N, D)
        else:
            y = R.shift_tokens(ln)
        nxt = dy[..., :half]
        if mutant == "last_row_grad_kept":
            nxt = nxt.reshape(B * N, half).roll(-1, 0).reshape(B, N, half)
        else:
            nxt = torch.cat((nxt[:, 1:], torch.zeros_like(nxt[:, :1])), dim=1)
        e = torch.cat((nxt, dy[..., half:]), dim=-1)
    dx, dw = _ln_bwd(e, g, xh, rs)
    if ds is not None:
        dx = dx + ds
    return dict(y=y, s=s, mean=mu.reshape(-1), rstd=rs.reshape(-1),
                dx=rnd(dx), dw=rnd(dw))


def ln_oracle(x, res, g, dy, ds, shift, eps=1e-5):
    x = x.to(F64).requires_grad_(True)
    g = g.to(F64).requires_grad_(True)
    s = x + res.to(F64) if res is not None else x
    y = R.ln_shift(s, g, shift, eps)
    outs, grads = [y], [dy.to(F64)]
    if ds is not None:
        outs.append(s)
        grads.append(ds.to(F64))
    torch.autograd.backward(outs, grads)
    sd = s.detach()
    mu, rs = _ln_stats(sd, eps)
    return dict(y=y.detach(), s=sd, mean=mu.reshape(-1), rstd=rs.reshape(-1),
                dx=x.grad, dw=g.grad)


# (B, N, D): D of the issue at three row shapes, and R = 1035 > the 1024
# blocks of the backward at D = 32; LN_SLOW[dtype] are the last fast-path
# and the first ragged slow-path widths
LN_ROWS = [(2, 32), (5, 1), (3, 2)]
LN_WIDE = {BF16: (2048, 2064), F32: (1024, 1040)}
LN_OFFSET_SHAPE = (2, 32, 512)


def ln_shapes(dtype):
    ds = [16, 48, 128, *LN_WIDE[dtype]]
    return [(b, n, d) for d in ds for (b, n) in LN_ROWS] + [(3, 345, 32)]


# variants: (shift, with res, with ds)
LN_VARIANTS = [(True, False, False), (False, False, False),
               (True, True, True), (False, True, True), (True, True, False)]


def ln_cases(dtype, with_res=None):
    """cases of ln_shift (with_res False), ln_shift_res (True) or both; the
    two entry points are two families, because the rounded s = x + res
    moves the statistics of the second by a bf16 ulp of its inputs"""
    cases = [(dname(dtype), b, n, d, sh, rs, ds, 0.0)
             for (b, n, d) in ln_shapes(dtype) for (sh, rs, ds) in LN_VARIANTS]
    b, n, d = LN_OFFSET_SHAPE
    cases += [(dname(dtype), b, n, d, True, False, False, 10.0),
              (dname(dtype), b, n, d, False, True, True, 10.0)]
    return [c for c in cases if with_res is None or c[5] == with_res]


def ln_family(case):
    return "ln_res" if case[5] else "ln"


def _dt(name):
    return {"bf16": BF16, "fp32": F32}[name]


@functools.lru_cache(maxsize=None)
def ln_inputs(case):
    dn, B, N, D, shift, with_res, with_ds, offset = case
    dtype = _dt(dn)
    g = _gen(1000 + B * 7 + N * 13 + D)
    x = _randn(g, B, N, D) + offset
    res = _randn(g, B, N, D) if with_res else None
    if with_res and offset:
        x, res = x - 3.0, res + 3.0   # both addends off centre, sum at offset
    inp = dict(x=x.to(dtype), res=None if res is None else res.to(dtype),
               g=_randn(g, D).to(dtype), dy=_randn(g, B, N, D).to(dtype),
               ds=_randn(g, B, N, D).to(dtype) if with_ds else None,
               shift=shift)
    return inp


def _cast(inp, dt):
    return {k: (v.to(dt) if torch.is_tensor(v) and v.is_floating_point() else v)
            for k, v in inp.items()}


def _rnd(dn, dt):
    """the kernel's storage rounding for the fp32 emulation of a ``dn``
    case; none when the formulas run in fp64"""
    return rounder(_dt(dn)) if dt == F32 else ident


def ln_emulate(case, mutant=None, dt=F32):
    inp = _cast(ln_inputs(case), dt)
    return ln_explicit(**inp, rnd=_rnd(case[0], dt), mutant=mutant)


def ln_errors(got, want, case):
    errs = {k: row_err(got[k], want[k]) for k in ("y", "dx")}
    errs["dw"] = row_err(got["dw"].reshape(1, -1), want["dw"].reshape(1, -1))
    if case[5]:
        errs["s"] = row_err(got["s"], want["s"])
    errs["mean"] = elem_err(got["mean"], want["mean"])
    errs["rstd"] = elem_err(got["rstd"], want["rstd"])
    return errs


# ---------------------------------------------------------------------------
# glu / gelu
# ---------------------------------------------------------------------------

def gelu_tanh_parts(g, mutant=None, fast=False):
    """value and derivative of tanh-GELU. ``fast``: tanh as common.h's
    fast_tanh forms it, (e - 1) / (e + 1) with e = exp(2x) and x clamped to
    +-15, every step rounded to the working precision — in fp32 its 1 + t
    and 1 - t^2 cancel a few times worse than with a correctly rounded
    tanh, which is the kernels' arithmetic and not a defect."""
    if mutant == "erf":
        cdf = 0.5 * (1 + torch.erf(g / math.sqrt(2)))
        pdf = torch.exp(-0.5 * g * g) / math.sqrt(2 * math.pi)
        return g * cdf, cdf + g * pdf
    k0, k1 = math.sqrt(2 / math.pi), 0.044715
    inner = k0 * (g + k1 * g * g * g)
    if mutant == "no_clamp" or fast:
        # without the +-15 clamp exp overflows: inf / inf
        e = torch.exp(2 * (inner if mutant == "no_clamp"
                           else inner.clamp(-15.0, 15.0)))
        t = (e - 1) / (e + 1)
    else:
        t = torch.tanh(inner)
    val = 0.5 * g * (1 + t)
    grad = 0.5 * (1 + t) + 0.5 * g * (1 - t * t) * k0 * (1 + 3 * k1 * g * g)
    return val, grad


def glu_explicit(h, dy, rnd=ident, mutant=None, fast=False):
    a, g = h.chunk(2, dim=-1)
    if mutant == "halves_swapped":
        a, g = g, a
    val, grad = gelu_tanh_parts(g, mutant, fast)
    da, dg = rnd(dy * val), rnd(dy * a * grad)
    if mutant == "halves_swapped":
        da, dg = dg, da
    return dict(y=rnd(a * val), dh=torch.cat((da, dg), dim=-1))


def gelu_explicit(h, dy, rnd=ident, mutant=None, fast=False):
    val, grad = gelu_tanh_parts(h, mutant, fast)
    return dict(y=rnd(val), dh=rnd(dy * grad))


def _act_oracle(fn, h, dy):
    h = h.to(F64).requires_grad_(True)
    y = fn(h)
    y.backward(dy.to(F64))
    return dict(y=y.detach(), dh=h.grad)


def glu_oracle(h, dy):
    return _act_oracle(R.glu_gelu, h, dy)


def gelu_oracle(h, dy):
    return _act_oracle(R.gelu, h, dy)


def gate_sweep(n):
    """``n`` gate values over [-30, 30]: an even grid plus +-0, the points
    where fast_tanh's argument crosses its +-15 clamp (|g| ~ 6.2) and the
    grid's neighbours of zero."""
    grid = torch.linspace(-30, 30, n - 8, dtype=F32)
    extra = torch.tensor([0.0, -0.0, 6.2, -6.2, 6.25, -6.25, 1e-3, -1e-3])
    return torch.cat((grid, extra))


# GLU: (rows, half width); the binding wants the full width a multiple of
# 16, so the narrowest fp32 row is half width 8 (two active threads) and
# the first fp32 width with two column blocks is 1032 (Hv = 258)
GLU_SHAPES = {BF16: [(4100, 8), (2050, 2056)], F32: [(4100, 8), (2050, 1032)]}
# GELU numel: more than 2048 * 256 vectors, a ragged few into the stride loop
GELU_NUMEL = {BF16: 8 * (2048 * 256 + 3), F32: 4 * (2048 * 256 + 6)}
SWEEP_N = 1024


def glu_cases(dtype):
    return [(dname(dtype), "shape", r, h) for r, h in GLU_SHAPES[dtype]] + \
        [(dname(dtype), "sweep", 16, SWEEP_N)]


@functools.lru_cache(maxsize=None)
def glu_inputs(case):
    dn, kind, rows, H = case
    dtype = _dt(dn)
    g = _gen(2000 + rows + H)
    h = _randn(g, rows, 2 * H)
    if kind == "sweep":
        h[:, H:] = gate_sweep(H)[torch.randperm(H, generator=g)]
    return dict(h=h.to(dtype), dy=_randn(g, rows, H).to(dtype))


def gelu_cases(dtype):
    return [(dname(dtype), "big", GELU_NUMEL[dtype]),
            (dname(dtype), "sweep", 16 * SWEEP_N)]


@functools.lru_cache(maxsize=None)
def gelu_inputs(case):
    dn, kind, numel = case
    dtype = _dt(dn)
    g = _gen(2100 + numel % 997)
    if kind == "sweep":
        h = gate_sweep(SWEEP_N).repeat(16, 1)
        dy = _randn(g, 16, SWEEP_N)
    else:
        # rows of 8 so that row_err sees every vector on its own scale
        h, dy = _randn(g, numel // 8, 8) * 2, _randn(g, numel // 8, 8)
    return dict(h=h.to(dtype), dy=dy.to(dtype))


def act_errors(got, want, case=None):
    return {k: row_err(got[k], want[k]) for k in ("y", "dh")}


# ---------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------

def ce_explicit(logits, targets, dnll, rnd=ident, mutant=None):
    x = logits
    V = x.shape[-1]
    m = x.amax(-1, keepdim=True)
    if mutant == "no_max_sub":
        m = torch.zeros_like(m)
    lse = torch.log(torch.exp(x - m).sum(-1, keepdim=True)) + m
    nll = (lse - x.gather(-1, targets[:, None])).squeeze(-1)
    hot = targets if mutant != "onehot_plus1" else (targets + 1) % V
    onehot = F.one_hot(hot, V).to(x.dtype)
    dl = rnd(dnll[:, None].to(x.dtype) * (torch.exp(x - lse) - onehot))
    return dict(nll=nll, lse=lse.squeeze(-1), dlogits=dl)


def ce_oracle(logits, targets, dnll):
    x = logits.to(F64).requires_grad_(True)
    logp = F.log_softmax(x, dim=-1)
    nll = -logp.gather(-1, targets[:, None]).squeeze(-1)
    nll.backward(dnll.to(F64))
    return dict(nll=nll.detach(), lse=torch.logsumexp(x.detach(), -1),
                dlogits=x.grad)


CE_V = [1, 7, 64, 65, 256, 1000]
CE_R = [1, 5, 99]


def ce_cases(dtype):
    cases = [(dname(dtype), "rand", r, v) for v in CE_V for r in CE_R]
    if dtype == F32:
        cases.append(("fp32", "extreme", 4, 256))
    return cases


@functools.lru_cache(maxsize=None)
def ce_inputs(case):
    dn, kind, Rr, V = case
    dtype = _dt(dn)
    g = _gen(3000 + Rr * 31 + V)
    if kind == "extreme":
        x = torch.full((Rr, V), -80.0)
        x[0, 17] = 80.0           # one logit at +80, the rest at -80
        x[1] = 3.25               # all equal
        x[2] = -100.0
        x[2, V - 1] = 100.0       # exp(100) is beyond fp32
        x[3] = _randn(g, V) * 3
        targets = torch.tensor([17, 5, 0, 9])
        dnll = torch.tensor([1.0, -0.5, 2.0, 0.0])
    else:
        x = _randn(g, Rr, V) * 3
        targets = torch.randint(0, V, (Rr,), generator=g)
        targets[0] = 0
        if Rr > 1:
            targets[1] = V - 1
        if Rr > 2:
            targets[2] = x[2].argmax()
        dnll = _randn(g, Rr)
        if Rr > 3:
            dnll[3] = 0.0         # a masked row: dlogits must be exactly 0
    return dict(logits=x.to(dtype), targets=targets, dnll=dnll)


def ce_emulate(case, mutant=None, dt=F32):
    inp = ce_inputs(case)
    return ce_explicit(inp["logits"].to(dt), inp["targets"],
                       inp["dnll"].to(dt), rnd=_rnd(case[0], dt),
                       mutant=mutant)


def ce_errors(got, want, case=None):
    # nll and lse are absolute quantities of O(log V): a floor of 1 keeps a
    # row whose nll happens to be near 0 from demanding the impossible
    return dict(nll=elem_err(got["nll"], want["nll"], floor=1.0),
                lse=elem_err(got["lse"], want["lse"], floor=1.0),
                dlogits=row_err(got["dlogits"], want["dlogits"]))


# ---------------------------------------------------------------------------
# rope_qkv
# ---------------------------------------------------------------------------

ROPE_SHAPES = [(1, 64, 1), (2, 64, 11), (3, 704, 2)]   # (B, N, H)


def rope_tables(n, dt=F32):
    """the fp32 tables the kernels are handed, viewed in ``dt``"""
    sin, cos = R.fixed_pos_embedding(n, 64, dtype=F32)
    return sin.to(dt), cos.to(dt)


def rope_explicit(qkv, sin, cos, mutant=None):
    """qkv: (B, N, 3*H*64); sin/cos: at least (N, 64) rows, (B*N, 64) for
    the mutant that never wraps the position."""
    B, N, C = qkv.shape
    x = qkv.reshape(B, N, C // 64, 64)
    if mutant == "pos_bn":
        s, c = sin[:B * N].reshape(B, N, 1, 64), cos[:B * N].reshape(B, N, 1, 64)
    else:
        s, c = sin[:N].reshape(1, N, 1, 64), cos[:N].reshape(1, N, 1, 64)
    return (x * c + R.rotate_every_two(x) * s).reshape(B, N, C)


@functools.lru_cache(maxsize=None)
def rope_inputs(shape):
    B, N, H = shape
    return (_randn(_gen(4000 + N + H), B, N, 3 * H * 64)).to(BF16)


# ---------------------------------------------------------------------------
# local attention (rope_qkv + attn_fwd + attn_bwd)
# ---------------------------------------------------------------------------

def _inv_rot(t, sin, cos):
    # transpose of x*c + rotate_every_two(x)*s
    return t * cos - R.rotate_every_two(t) * sin


def attn_explicit(qkv, sin, cos, dout, H, wsz, halo=None, rnd=ident,
                  mutant=None):
    """The three attention kernels in formulas. Rounding points: the
    rotated q/k/v, the P operand of P.V and of dV = P^T dO, the dS operand
    of dQ and dK, out, dqkv. ``lse`` is max + log(sum) of the scaled
    logits, zero lookback keys included; ``dhalo`` stays fp32."""
    B, N, _ = qkv.shape
    dh, W = 64, N // wsz
    sin, cos = sin.to(qkv.dtype), cos.to(qkv.dtype)

    def heads(t):
        return t.reshape(B, N, H, dh).transpose(1, 2)

    def rot(t):
        return rnd(t * cos + R.rotate_every_two(t) * sin)

    q, k, v = map(heads, qkv.chunk(3, dim=-1))
    q, k = rot(q), rot(k)
    v = rnd(v) if mutant == "v_not_rotated" else rot(v)

    def win(t):
        return t.reshape(B, H, W, wsz, dh)

    def band(t, h):
        if h is None:
            first = torch.zeros_like(t[:, :, :1])
        else:
            first = h.reshape(B, wsz, H, dh).permute(0, 2, 1, 3).unsqueeze(2)
        return torch.cat((torch.cat((first, t[:, :, :-1]), dim=2), t), dim=3)

    hk = hv = None
    if halo is not None:
        hk, hv = halo[..., :H * dh], halo[..., H * dh:]
    qw, kb, vb = win(q), band(win(k), hk), band(win(v), hv)
    scale = dh ** -0.5

    diag = wsz + {"mask_minus1": -1, "mask_plus1": 1}.get(mutant, 0)
    mask = torch.ones(wsz, 2 * wsz, dtype=torch.bool).tril(diag)
    if mutant == "oldest_dropped":
        mask[:, 0] = False
    mask = mask.expand(W, wsz, 2 * wsz).clone()
    if mutant == "no_zero_quirk" and halo is None:
        mask[0, :, :wsz] = False

    sim = torch.einsum("bhwid,bhwjd->bhwij", qw, kb) * scale
    sim = sim.masked_fill(~mask, -math.inf)
    m = sim.amax(-1, keepdim=True)
    p = torch.exp(sim - m)
    l = p.sum(-1, keepdim=True)
    lse = m + torch.log(l)
    o = torch.einsum("bhwij,bhwjd->bhwid", rnd(p), vb) / l
    out = rnd(o.permute(0, 2, 3, 1, 4).reshape(B, N, H * dh))

    def to_win(t):   # (B, N, H*dh) -> (B, H, W, wsz, dh)
        return t.reshape(B, W, wsz, H, dh).permute(0, 3, 1, 2, 4)

    ow, dow = to_win(out), to_win(dout)
    delta = (ow * dow).sum(-1, keepdim=True)
    P = torch.exp(sim - lse)
    dvb = torch.einsum("bhwij,bhwid->bhwjd", rnd(P), dow)
    dP = torch.einsum("bhwid,bhwjd->bhwij", dow, vb)
    dS = rnd(P * (dP - delta))
    dq = torch.einsum("bhwij,bhwjd->bhwid", dS, kb) * scale
    dkb = torch.einsum("bhwij,bhwid->bhwjd", dS, qw) * scale

    def fold(db):
        own, look = db[:, :, :, wsz:].clone(), db[:, :, :, :wsz]
        own[:, :, :-1] += look[:, :, 1:]
        return own.reshape(B, H, N, dh), look[:, :, 0]

    dk, dhk = fold(dkb)
    dv, dhv = fold(dvb)
    dq = _inv_rot(dq.reshape(B, H, N, dh), sin, cos)
    dk = _inv_rot(dk, sin, cos)
    if mutant != "v_not_rotated":
        dv = _inv_rot(dv, sin, cos)

    def merge(t):    # (B, H, N, dh) -> (B, N, H*dh)
        return t.transpose(1, 2).reshape(B, N, H * dh)

    res = dict(out=out, lse=lse.reshape(B, H, N),
               dqkv=rnd(torch.cat((merge(dq), merge(dk), merge(dv)), dim=-1)))
    if halo is not None:
        def hm(t):   # (B, H, wsz, dh) -> (B, wsz, H*dh)
            return t.transpose(1, 2).reshape(B, wsz, H * dh)
        res["dhalo"] = torch.cat((hm(dhk), hm(dhv)), dim=-1)
    return res


def attn_oracle(qkv, sin, cos, dout, H, wsz, halo=None):
    """reference.local_attention in fp64 with autograd; lse (which the
    reference does not expose) and the halo form from the explicit
    formulas in fp64, which test_kernel_oracle.py holds to the reference."""
    ex = attn_explicit(qkv.to(F64), sin.to(F64), cos.to(F64), dout.to(F64),
                       H, wsz, None if halo is None else halo.to(F64))
    if halo is not None:
        return ex
    x = qkv.to(F64).requires_grad_(True)
    out = R.local_attention(x, sin.to(F64), cos.to(F64), H, wsz)
    out.backward(dout.to(F64))
    return dict(out=out.detach(), lse=ex["lse"], dqkv=x.grad)


ATTN_SHAPES = [(2, 256, 3, 128), (1, 384, 1, 192), (1, 640, 2, 320),
               (1, 192, 2, 192)]


def attn_cases():
    cases = [("rand", s, shape) for shape in ATTN_SHAPES for s in (0.125, 1.0)]
    # one dominant key per window: early in the band of the next window's
    # rows (tile 0), or in the last 64-key tile of its own window's rows
    cases += [("hot_first", 0.125, (1, 384, 2, 192)),
              ("hot_last", 0.125, (1, 384, 2, 192))]
    return cases


@functools.lru_cache(maxsize=None)
def attn_inputs(case):
    kind, scale, (B, N, H, wsz) = case
    g = _gen(5000 + N + 3 * H + wsz + (7 if scale == 1.0 else 0))
    sin, cos = rope_tables(N)
    x = _randn(g, B, N, 3 * H * 64) * scale
    if kind != "rand":
        # build in rotated space, then rotate back: every q leans 2 along a
        # common direction u and the hot key of each window is 24 u, a
        # logit of about 6 above noise of about 0.02
        u = F.normalize(_randn(g, 64), dim=0)
        xr = x.reshape(B, N, 3 * H, 64)
        xr[:, :, :H] += 2.0 * u
        off = 0 if kind == "hot_first" else wsz - 30
        xr[:, off::wsz, H:2 * H] = 24.0 * u
        x = _inv_rot(xr, sin.reshape(1, N, 1, 64), cos.reshape(1, N, 1, 64)) \
            .reshape(B, N, 3 * H * 64)
    dout = _randn(g, B, N, H * 64) * scale
    return dict(qkv=x.to(BF16), sin=sin, cos=cos, dout=dout.to(BF16), H=H,
                wsz=wsz)


# halo: the joined sequence of two virtual ranks, wsz 192, two windows each
HALO_SHAPE = (1, 768, 2, 192)


@functools.lru_cache(maxsize=None)
def halo_inputs():
    """second rank's inputs: its half of the joined sequence and the bf16
    rotated [k|v] of the first rank's last window"""
    B, N, H, wsz = HALO_SHAPE
    g = _gen(5900)
    sin, cos = rope_tables(N)
    x = (_randn(g, B, N, 3 * H * 64) * 0.5).to(BF16)
    dout = (_randn(g, B, N, H * 64) * 0.5).to(BF16)
    L = N // 2
    tail = x[:, L - wsz:L].float().reshape(B, wsz, 3 * H, 64)[:, :, H:]
    s, c = sin[L - wsz:L].reshape(1, wsz, 1, 64), cos[L - wsz:L].reshape(1, wsz, 1, 64)
    halo = (tail * c + R.rotate_every_two(tail) * s).reshape(B, wsz, 2 * H * 64)
    return dict(joined=dict(qkv=x, sin=sin, cos=cos, dout=dout, H=H, wsz=wsz),
                second=dict(qkv=x[:, L:].contiguous(), sin=sin[L:].contiguous(),
                            cos=cos[L:].contiguous(),
                            dout=dout[:, L:].contiguous(), H=H, wsz=wsz,
                            halo=halo.to(BF16)))


def attn_emulate(inp, mutant=None, dt=F32):
    return attn_explicit(**_cast(inp, dt), rnd=_rnd("bf16", dt),
                         mutant=mutant)


def attn_errors(got, want, inp):
    H = inp["H"]
    B, N, _ = want["out"].shape
    errs = dict(
        out=row_err(got["out"].reshape(B, N, H, 64), want["out"].reshape(B, N, H, 64)),
        lse=elem_err(got["lse"], want["lse"], floor=1.0),
        dqkv=row_err(got["dqkv"].reshape(B, N, 3 * H, 64),
                     want["dqkv"].reshape(B, N, 3 * H, 64)))
    if "dhalo" in want:
        w = want["dhalo"].shape[1]
        errs["dhalo"] = row_err(got["dhalo"].reshape(B, w, 2 * H, 64),
                                want["dhalo"].reshape(B, w, 2 * H, 64))
    return errs


# ---------------------------------------------------------------------------
# SGU
# ---------------------------------------------------------------------------

def _sgu_w(w, mutant):
    k = {"tril_minus1": -1, "tril_plus1": 1}.get(mutant, 0)
    wl = w.tril(k).clone()
    if mutant == "skip_ktile" and w.shape[0] > 256:
        wl[256:, 64:128] = 0
    return wl


def sgu_direct_explicit(xa, g_ln, w, bias, t, rnd=ident, mutant=None):
    """sgu_fwd, sgu_dgate and sgu_dw on the inputs they are handed.
    Rounding points: out, gate_out, dg; dW stays fp32."""
    N = w.shape[0]
    wl = _sgu_w(w, mutant)
    go = torch.einsum("bnd,mn->bmd", g_ln, wl)
    if mutant != "no_bias":
        go = go + bias.reshape(1, N, 1)
    tt, gg = t, g_ln
    if mutant == "dw_first_chunk_only":
        tt, gg = t[..., :768], g_ln[..., :768]
    return dict(out=rnd(xa * go), gate_out=rnd(go),
                dg=rnd(torch.einsum("bmd,mn->bnd", t, wl)),
                dw=torch.einsum("bmd,bnd->mn", tt, gg).tril())


def sgu_direct_oracle(xa, g_ln, w, bias, t):
    return sgu_direct_explicit(xa.to(F64), g_ln.to(F64), w.to(F64),
                               bias.to(F64), t.to(F64))


def sgu_e2e_explicit(x, gw, w, bias, dy, eps=1e-5, rnd=ident, mutant=None,
                     composite=False):
    """functional.sgu_gate forward and backward. Rounding points on top of
    the direct kernels': g_ln (the LN kernel's output), t = dy * xa, the
    saved gate_out that feeds dxa, dW and db cast to bf16, and the LN
    backward's outputs. ``composite``: the N < 256 path, whose matmul
    result is rounded before the bias is added."""
    xa, gate = x.chunk(2, dim=-1)
    N = x.shape[1]
    mu, rs = _ln_stats(gate, eps)
    xh = (gate - mu) * rs
    g_ln = rnd(xh * gw)
    wl = _sgu_w(w, mutant)
    go = torch.einsum("bnd,mn->bmd", g_ln, wl)
    if composite:
        go = rnd(go)
    if mutant != "no_bias":
        go = go + bias.reshape(1, N, 1)
    if composite:
        go = rnd(go)
    out = rnd(xa * go)
    t = rnd(dy * xa)
    dxa = rnd(dy * rnd(go))
    dg_ln = rnd(torch.einsum("bmd,mn->bnd", t, wl))
    tt, gg = t, g_ln
    if mutant == "dw_first_chunk_only":
        tt, gg = t[..., :768], g_ln[..., :768]
    dW = rnd(torch.einsum("bmd,bnd->mn", tt, gg).tril())
    db = rnd(t.sum(dim=(0, 2))).reshape(bias.shape)
    dgate, dgw = _ln_bwd(dg_ln, gw, xh, rs)
    return dict(out=out, dxa=dxa, dgate=rnd(dgate), dgw=rnd(dgw), dW=dW, db=db)


def sgu_e2e_oracle(x, gw, w, bias, dy, eps=1e-5):
    x, gw, w, bias = (t.to(F64).requires_grad_(True) for t in (x, gw, w, bias))
    out = R.sgu_gate(x, gw, w, bias, eps)
    out.backward(dy.to(F64))
    d2 = x.shape[-1] // 2
    return dict(out=out.detach(), dxa=x.grad[..., :d2], dgate=x.grad[..., d2:],
                dgw=gw.grad, dW=w.grad, db=bias.grad)


SGU_SHAPES = [(2, 512, 64), (1, 768, 64), (1, 256, 832), (2, 512, 832)]
SGU_COMPOSITE_SHAPE = (2, 128, 64)


@functools.lru_cache(maxsize=None)
def sgu_inputs(shape):
    """W ~ N^-0.5 with a full upper triangle and a random bias, so that the
    spatial matmul is the gate and not a perturbation of bias = 1."""
    B, N, D = shape
    g = _gen(6000 + N + D + B)
    x = (_randn(g, B, N, 2 * D) / 2).to(BF16)
    gw = (1 + 0.25 * _randn(g, D)).to(BF16)
    w = (_randn(g, N, N) * N ** -0.5).to(BF16)
    bias = (0.5 * _randn(g, N, 1)).to(BF16)
    dy = (_randn(g, B, N, D) / 2).to(BF16)
    # the direct kernels' own operands, as the forward would hand them over
    xa = x[..., :D].contiguous()
    gate = x[..., D:].float()
    mu, rs = _ln_stats(gate, 1e-5)
    g_ln = ((gate - mu) * rs * gw.float()).to(BF16)
    t = (dy.float() * xa.float()).to(BF16)
    return dict(e2e=dict(x=x, gw=gw, w=w, bias=bias, dy=dy),
                direct=dict(xa=xa, g_ln=g_ln, w=w, bias=bias.reshape(N), t=t))


def sgu_direct_errors(got, want, inp=None):
    errs = {k: row_err(got[k], want[k]) for k in ("out", "gate_out", "dg")}
    errs["dw"] = row_err(got["dw"].tril(), want["dw"])
    return errs


def sgu_e2e_errors(got, want, inp=None):
    errs = {k: row_err(got[k], want[k]) for k in ("out", "dxa", "dgate")}
    errs["dgw"] = row_err(got["dgw"].reshape(1, -1), want["dgw"].reshape(1, -1))
    errs["dW"] = row_err(got["dW"].tril(), want["dW"])
    errs["db"] = elem_err(got["db"], want["db"])
    return errs


# ---------------------------------------------------------------------------
# fused_adamw / grad_sumsq
# ---------------------------------------------------------------------------

ADAMW_HP = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2)
ADAMW_GRAD_SCALE, ADAMW_CLIP, ADAMW_STEPS = 0.25, 0.5, 3
ADAMW_NCHUNKS = 2100
_CHUNK_LENS = [0, 1, 24, 257, 7, 64, 300, 8, 255, 33]


@functools.lru_cache(maxsize=None)
def adamw_inputs(dn, sharded):
    """2100 ragged chunks with small gaps between them over one flat
    buffer. ``sharded``: the fp32 state covers only [lo, hi) of it, lo in
    the middle of a chunk, and the tables are clipped to that range."""
    dtype = _dt(dn)
    g = _gen(7000 + (1 if sharded else 0))
    starts, ends, pos = [], [], 3
    for c in range(ADAMW_NCHUNKS):
        n = _CHUNK_LENS[c % len(_CHUNK_LENS)]
        starts.append(pos)
        ends.append(pos + n)
        pos += n + (c % 3)
    P = pos + 5
    starts, ends = torch.tensor(starts), torch.tensor(ends)
    decay = (torch.arange(ADAMW_NCHUNKS) % 3 != 0).to(torch.int32)
    lo, hi = 0, P
    if sharded:
        lo, hi = int(starts[13]) + 100, int(ends[ADAMW_NCHUNKS - 8]) - 3
        starts, ends = starts.clamp(lo, hi), ends.clamp(lo, hi)
        keep = ends > starts
        starts, ends, decay = starts[keep], ends[keep], decay[keep]
    master = _randn(g, P)
    grads = [(_randn(g, P) * (1 + 3 * torch.rand(P, generator=g))).to(dtype)
             for _ in range(ADAMW_STEPS)]
    return dict(P=P, lo=lo, hi=hi, starts=starts, ends=ends, decay=decay,
                master=master, params=master.to(dtype), grads=grads,
                exp_avg=0.1 * _randn(g, P), exp_avg_sq=0.01 * _randn(g, P) ** 2)


def adamw_explicit(inp, dt, param_rnd=ident, mutant=None):
    """The plain AdamW formula over the chunks, ADAMW_STEPS steps from
    step 1. In fp32 the hyper-parameters are the floats the kernel is
    handed, as is 1 - b^t. Elements outside every chunk keep their values.
    State tensors are full length; the caller slices [lo, hi)."""
    P = inp["P"]
    hp = {k: torch.tensor(v, dtype=F64).to(dt) for k, v in ADAMW_HP.items()}
    cov = torch.zeros(P, dtype=torch.bool)
    wdv = torch.zeros(P, dtype=dt)
    for s, e, d in zip(inp["starts"].tolist(), inp["ends"].tolist(),
                       inp["decay"].tolist()):
        cov[s:e] = True
        if d or mutant == "decay_everywhere":
            wdv[s:e] = hp["wd"]
    p, m, v = (inp[k].to(dt).clone() for k in ("master", "exp_avg", "exp_avg_sq"))
    params = inp["params"].to(dt).clone()
    gs = 1.0 if mutant == "grad_scale_ignored" else ADAMW_GRAD_SCALE
    one = torch.tensor(1.0, dtype=dt)
    for step in range(1, ADAMW_STEPS + 1):
        g = inp["grads"][step - 1].to(dt) * torch.tensor(gs * ADAMW_CLIP, dtype=dt)
        bc1 = one - hp["b1"] ** step
        bc2 = one - hp["b2"] ** step
        if mutant == "no_bias_correction":
            bc1 = bc2 = one
        m2 = hp["b1"] * m + (one - hp["b1"]) * g
        v2 = hp["b2"] * v + (one - hp["b2"]) * g * g
        p2 = p - hp["lr"] * ((m2 / bc1) / (torch.sqrt(v2 / bc2) + hp["eps"]) + wdv * p)
        m, v, p = torch.where(cov, m2, m), torch.where(cov, v2, v), torch.where(cov, p2, p)
        params = torch.where(cov, param_rnd(p), params)
    return dict(master=p, exp_avg=m, exp_avg_sq=v, params=params)


def adamw_errors(got, want, inp):
    lo, hi = inp["lo"], inp["hi"]
    errs = {k: elem_err(got[k][lo:hi], want[k][lo:hi])
            for k in ("master", "exp_avg", "exp_avg_sq")}
    errs["params"] = elem_err(got["params"], want["params"])
    return errs


SUMSQ_NUMEL = [8, 8 * (2048 * 256 + 3)]


@functools.lru_cache(maxsize=None)
def sumsq_inputs(dn, numel):
    """the vectors past the first trip of 2048 blocks are four times as
    loud, so that losing them costs 1e-4 of the sum"""
    x = _randn(_gen(7100 + numel % 991), numel) * 3
    x[2048 * 256 * 8:] *= 4
    return x.to(_dt(dn))


def sumsq_emulate(x, order=None):
    """fp32 in the kernel's order: each thread sums the squares of its
    vectors, 64 lanes and 4 waves join, and the blocks' partials are added
    to one float one after the other (atomicAdd) in ``order``, a
    permutation of the blocks; in block order by default."""
    vlen = 8 if x.dtype == BF16 else 4
    nv = x.numel() // vlen
    grid = min((nv + 255) // 256, 2048)
    T = grid * 256
    iters = (nv + T - 1) // T
    sq = torch.zeros(iters * T, vlen, dtype=F32)
    sq[:nv] = x.float().reshape(nv, vlen) ** 2
    acc = torch.zeros(T, dtype=F32)
    for it in range(iters):
        for j in range(vlen):
            acc = acc + sq[it * T:(it + 1) * T, j]
    blocks = acc.reshape(grid, 256).sum(1)
    if order is not None:
        blocks = blocks[order]
    tot = torch.zeros((), dtype=F32)
    for b in blocks:        # cumsum would accumulate in fp64 on the CPU
        tot = tot + b
    return tot


def sumsq_orders(x):
    """the atomicAdd order is the hardware's: block order, its reverse and
    six seeded shuffles stand for it"""
    vlen = 8 if x.dtype == BF16 else 4
    grid = min((x.numel() // vlen + 255) // 256, 2048)
    g = _gen(7200)
    idx = torch.arange(grid)
    return [idx, idx.flip(0)] + [torch.randperm(grid, generator=g)
                                 for _ in range(6)]


def sumsq_oracle(x):
    return (x.to(F64) ** 2).sum()


# ---------------------------------------------------------------------------
# fp8 quantization
# ---------------------------------------------------------------------------

FP8_SHAPES = [(66, 70), (2, 8), (130, 64)]
FP8_SCALE = 0.03125 * 1.3   # not a power of two: 1/scale is inexact


@functools.lru_cache(maxsize=None)
def fp8_inputs(shape):
    """values/scale spread over the e4m3 range, with planted classes:
    beyond +-448, +-0, the e4m3 subnormals (multiples of 2^-9 below 2^-6)
    and the halfway points between them"""
    r, c = shape
    g = _gen(8000 + r + c)
    t = _randn(g, r, c) * 100 * FP8_SCALE
    flat = t.reshape(-1)
    sub = torch.arange(0, 17, dtype=F32) * 2.0 ** -10 * FP8_SCALE
    plant = torch.cat((torch.tensor([460.0, -460.0, 1e4, -1e4, 448.0, -448.0,
                                     0.0, -0.0]) * FP8_SCALE, sub, -sub))
    n = min(plant.numel(), flat.numel())
    idx = torch.randperm(flat.numel(), generator=g)[:n]
    flat[idx] = plant[:n]
    return t.to(BF16), torch.tensor([FP8_SCALE], dtype=F32)


def fp8_reference(t, scale, divide=False):
    """bytes of clamp(t * (1/scale)) in e4m3 — the kernel's form — or of
    clamp(t / scale), the form the existing 0.1 % cap is stated for"""
    tf = t.float().cpu()
    s = scale.float().cpu()
    y = tf / s if divide else tf * (1.0 / s)
    return y.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)


# ---------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------

def _worst(pairs):
    worst = {}
    for errs in pairs:
        for k, v in errs.items():
            worst[k] = max(worst.get(k, 0.0), v)
    return {k: (v, MARGIN * v) for k, v in worst.items()}


@functools.lru_cache(maxsize=None)
def ln_oracle_of(case):
    return ln_oracle(**ln_inputs(case))


@functools.lru_cache(maxsize=None)
def glu_oracle_of(case):
    return glu_oracle(**glu_inputs(case))


@functools.lru_cache(maxsize=None)
def gelu_oracle_of(case):
    return gelu_oracle(**gelu_inputs(case))


@functools.lru_cache(maxsize=None)
def ce_oracle_of(case):
    return ce_oracle(**ce_inputs(case))


@functools.lru_cache(maxsize=None)
def attn_oracle_of(case):
    return attn_oracle(**attn_inputs(case))


@functools.lru_cache(maxsize=None)
def halo_oracle():
    return attn_oracle(**halo_inputs()["second"])


@functools.lru_cache(maxsize=None)
def sgu_direct_oracle_of(shape):
    return sgu_direct_oracle(**sgu_inputs(shape)["direct"])


@functools.lru_cache(maxsize=None)
def sgu_e2e_oracle_of(shape):
    return sgu_e2e_oracle(**sgu_inputs(shape)["e2e"])


@functools.lru_cache(maxsize=None)
def adamw_oracle_of(dn, sharded):
    return adamw_explicit(adamw_inputs(dn, sharded), F64)


def adamw_emulate(dn, sharded, mutant=None, dt=F32):
    return adamw_explicit(adamw_inputs(dn, sharded), dt,
                          param_rnd=_rnd(dn, dt), mutant=mutant)


def sgu_direct_emulate(shape, mutant=None, dt=F32):
    return sgu_direct_explicit(**_cast(sgu_inputs(shape)["direct"], dt),
                               rnd=_rnd("bf16", dt),
                               mutant=mutant)


def sgu_e2e_emulate(shape, mutant=None, dt=F32, composite=False):
    return sgu_e2e_explicit(**_cast(sgu_inputs(shape)["e2e"], dt),
                            rnd=_rnd("bf16", dt),
                            mutant=mutant, composite=composite)


def act_emulate(kind, case, mutant=None, dt=F32):
    inputs, explicit = (glu_inputs, glu_explicit) if kind == "glu" else \
        (gelu_inputs, gelu_explicit)
    return explicit(**_cast(inputs(case), dt), rnd=_rnd(case[0], dt),
                    mutant=mutant, fast=(dt == F32))


@functools.lru_cache(maxsize=None)
def bounds(family: str, dn: str = "bf16"):
    """{output: (emulation error, bound)} for one family and dtype"""
    dtype = _dt(dn)
    if family in ("ln", "ln_res"):
        return _worst(ln_errors(ln_emulate(c), ln_oracle_of(c), c)
                      for c in ln_cases(dtype, family == "ln_res"))
    if family == "glu":
        return _worst(act_errors(act_emulate("glu", c), glu_oracle_of(c))
                      for c in glu_cases(dtype))
    if family == "gelu":
        return _worst(act_errors(act_emulate("gelu", c), gelu_oracle_of(c))
                      for c in gelu_cases(dtype))
    if family == "ce":
        return _worst(ce_errors(ce_emulate(c), ce_oracle_of(c))
                      for c in ce_cases(dtype))
    if family == "attn":
        return _worst(attn_errors(attn_emulate(attn_inputs(c)),
                                  attn_oracle_of(c), attn_inputs(c))
                      for c in attn_cases())
    if family == "attn_halo":
        inp = halo_inputs()["second"]
        return _worst([attn_errors(attn_emulate(inp), halo_oracle(), inp)])
    if family == "sgu_direct":
        return _worst(sgu_direct_errors(sgu_direct_emulate(s),
                                        sgu_direct_oracle_of(s))
                      for s in SGU_SHAPES)
    if family == "sgu_e2e":
        return _worst(sgu_e2e_errors(sgu_e2e_emulate(s), sgu_e2e_oracle_of(s))
                      for s in SGU_SHAPES)
    if family == "sgu_composite":
        s = SGU_COMPOSITE_SHAPE
        return _worst([sgu_e2e_errors(sgu_e2e_emulate(s, composite=True),
                                      sgu_e2e_oracle_of(s))])
    if family == "adamw":
        return _worst(adamw_errors(adamw_emulate(dn, sh), adamw_oracle_of(dn, sh),
                                   adamw_inputs(dn, sh))
                      for sh in (False, True))
    if family == "sumsq":
        return _worst(
            dict(sumsq=elem_err(sumsq_emulate(sumsq_inputs(dn, n), o),
                                sumsq_oracle(sumsq_inputs(dn, n))))
            for n in SUMSQ_NUMEL for o in sumsq_orders(sumsq_inputs(dn, n)))
    raise KeyError(family)


def check(family, dn, errs, label=""):
    """print every figure, then hold each to its bound; returns the list of
    (output, measured, bound) that miss"""
    b = bounds(family, dn)
    missed = []
    for k, v in errs.items():
        emu, bound = b[k]
        print(f"KTOL|{family}|{k}|{dn}|{emu:.3e}|{bound:.3e}|{v:.3e}|{label}")
        if not v <= bound:
            missed.append((k, v, bound))
    return missed
