"""fp64 oracles, storage-precision emulations and mutants of the three
decode-step kernels (progen_amd/ops/hip/decode_{ln_shift,attn,sgu}_body.h),
by the method of tests/KERNEL_TOLERANCES.md. tests/test_decode_oracle.py
proves on the CPU that the bounds tell the emulation from every mutant;
tests/test_gpu_decode_kernel_edges.py runs the kernels. CPU only.

Three computations of every case, on the dtype-rounded inputs:

  oracle     ``reference.decode_ln_shift``, ``decode_attention`` and
             ``decode_sgu`` in fp64, on clones of the caches;
  emulation  the same formulas in fp32, rounded to bf16 exactly where the
             body calls ``round_trip<BF>`` or ``st8<BF>``:
               ln    the stored h + res, y, prev;
               attn  the rotated q, k, v before the scores, out;
               sgu   gl before the ``pos`` term and the history write, out;
             the fp32 instantiation rounds nothing;
  mutants    the emulation with one defect (``*_MUTANTS``: name -> the
             predicate of the cases it applies to).

The attention emulation has the kernel's structure: 32 lane groups, group g
taking band rows g, g + 32, ... in an online softmax of its own (running
maximum, ``exp(m - mn)`` rescale); group 0 seeded with the current row and,
while pos < window, with ``window`` zero logits; then the eight groups of a
wave joined under the wave's maximum and the four waves under the block's,
a group or wave without rows (m = -inf) entering with weight 0. It does not
claim fp32 bit-exactness: ``dec_attn`` leaves contraction to the compiler,
and the margin covers that.

The bound of a (family, output, dtype) is MARGIN x the emulation's
``row_err`` against the oracle, worst case over the family's cases; the
bf16 k / v row that ``dec_attn`` writes is held to one bf16 step instead.
``dec_ln`` with and without ``res`` are two families, as ``ln`` and
``ln_res`` are in kernel_oracle.py: the rounded sum moves the statistics.

Every cache row a step must not read holds NaN.
"""

from __future__ import annotations

import functools
import math

import torch

from kernel_oracle import (BF16, F32, F64, MARGIN, bf16_ulp_dist, dname,
                           ident, rope_tables, rounder, row_err)
from progen_amd.ops import reference as R

NAN = float("nan")
EPS = 1e-5
DTYPES = (BF16, F32)


def _dt(dn):
    return {"bf16": BF16, "fp32": F32}[dn]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F32)


def _rnd(dn, dt):
    """the kernel's storage rounding inside the fp32 emulation of a ``dn``
    case; none when the formulas run in fp64"""
    return rounder(_dt(dn)) if dt == F32 else ident


def _to(t, dt):
    return None if t is None else t.to(dt)


# ---------------------------------------------------------------------------
# dec_ln_shift
# ---------------------------------------------------------------------------

# 16: the narrowest row (two chunks, one per half); 2048 / 2064: the last
# width that keeps its chunk in registers (ONE) and the first that re-reads
# h, ragged: threads 0 and 1 own two chunks; 4096: two chunks a thread
LN_D = (16, 128, 2048, 2064, 4096)
LN_B = (1, 3)
# (shift, res, prev given)
LN_VARIANTS = ((True, True, True), (True, False, True), (False, True, True),
               (False, True, False), (False, False, False))


def ln_cases(dtype):
    """(dtype name, B, D, shift, res, prev)"""
    return [(dname(dtype), B, D, *v)
            for D in LN_D for B in LN_B for v in LN_VARIANTS]


def ln_family(case):
    return "dec_ln_res" if case[4] else "dec_ln"


@functools.lru_cache(maxsize=None)
def ln_inputs(case):
    """row b is 4**b times as loud as row 0 and sits at mean b: a per-row
    metric sees the quiet row, a global one would not"""
    dn, B, D, shift, res, prev = case
    dtype = _dt(dn)
    g = _gen(11000 + 7 * B + D)
    loud = (4.0 ** torch.arange(B, dtype=F32)).reshape(B, 1)
    off = torch.arange(B, dtype=F32).reshape(B, 1)
    h = _randn(g, B, D) * loud + off
    r = _randn(g, B, D) * loud
    gw = 1 + 0.25 * _randn(g, D)
    pv = _randn(g, B, D)
    return dict(h=h.to(dtype), res=r.to(dtype) if res else None,
                g=gw.to(dtype), prev=pv.to(dtype) if prev else None,
                shift=shift)


def ln_explicit(h, res, g, prev, shift, rnd=ident, mutant=None):
    """decode_ln_shift_body.h in formulas; returns y and the h and prev the
    kernel leaves behind (prev None when none was given)"""
    D = h.shape[-1]
    split = D // 2
    s = rnd(h + res) if res is not None else h
    st = s[:, :D - 8] if mutant == "stats_short" else s
    mu = st.mean(-1, keepdim=True)
    var = ((st - mu) ** 2).mean(-1, keepdim=True)
    ln = rnd((s - mu) * torch.rsqrt(var + EPS) * g)
    y = ln
    if shift:
        cut = split + 8 if mutant == "shift_late" else split
        y = torch.cat((prev[:, :cut], ln[:, cut:]), dim=-1)
    new_prev = None
    if prev is not None:
        new_prev = y if mutant == "prev_takes_y" else ln
    return dict(y=y, h=h if mutant == "h_not_updated" else s, prev=new_prev)


LN_MUTANTS = {
    # the shifted half ends one 8-element chunk late
    "shift_late": lambda c: c[3],
    # prev <- y: with a shift its first half keeps the old row
    "prev_takes_y": lambda c: c[3],
    # the sum is normalised but never stored
    "h_not_updated": lambda c: c[4],
    # mean and variance leave out the last chunk; at D <= 128 that is at
    # least 1/16 of the row
    "stats_short": lambda c: c[2] <= 128,
}


def ln_emulate(case, mutant=None, dt=F32):
    inp = {k: (_to(v, dt) if torch.is_tensor(v) else v)
           for k, v in ln_inputs(case).items()}
    return ln_explicit(**inp, rnd=_rnd(case[0], dt), mutant=mutant)


@functools.lru_cache(maxsize=None)
def ln_oracle(case):
    inp = ln_inputs(case)
    h = inp["h"].to(F64).clone()
    prev = None if inp["prev"] is None else inp["prev"].to(F64).clone()
    y = R.decode_ln_shift(h, _to(inp["res"], F64), inp["g"].to(F64), prev,
                          inp["shift"], EPS)
    return dict(y=y, h=h, prev=prev)


def ln_errors(got, want, case):
    """y always; h where a residual is added; prev where one is kept"""
    errs = dict(y=row_err(got["y"], want["y"]))
    if case[4]:
        errs["h"] = row_err(got["h"], want["h"])
    if case[5]:
        errs["prev"] = row_err(got["prev"], want["prev"])
    return errs


# ---------------------------------------------------------------------------
# dec_attn
# ---------------------------------------------------------------------------

ATTN_B, ATTN_H = 2, 3
GROUPS = 32            # DEC_ATTN_ROWS_PER_ITER: lane groups of a block
# (window, N, positions): nrows = pos - start in 0, 1, 7..9 (one wave
# partly filled), 31..33 (the last group's first row, group 0's second),
# 63..65, and 127..129 rows around one unrolled round of 4 x 32; every
# window start, its last row and the step from one lookback to the next
ATTN_POSITIONS = (
    (64, 256, (0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 191, 192,
               255)),
    (192, 384, (191, 192, 383)),
    (256, 512, (127, 128, 129, 255, 256, 383, 384, 385, 511)),
)
# peaked: q six times as loud and one cached key PEAK x the rotated q, a
# logit of about PEAK * 36 * 64 / 8 = 144 over others of about +-6 * 3: the
# weights of every other row underflow against it in fp32. At the band's
# first row the maximum is reached on group 0's first cached row and every
# later weight vanishes; at the last row (pos - 1) it arrives at the end of
# a group's chain and the sums gathered before it are rescaled away
ATTN_KINDS = ("rand", "peak_first", "peak_last")
PEAK = 0.5


def band(window, pos):
    """(start, nrows) of the cached rows [start, pos) a step reads"""
    w0 = (pos // window) * window
    start = max(w0 - window, 0)
    return start, pos - start


def attn_cases(dtype):
    """(dtype name, kind, window, N, pos)"""
    out = []
    for window, N, positions in ATTN_POSITIONS:
        for pos in positions:
            for kind in ATTN_KINDS:
                if kind != "rand" and band(window, pos)[1] == 0:
                    continue
                out.append((dname(dtype), kind, window, N, pos))
    return out


def _rot(t, sin_p, cos_p):
    return t * cos_p + R.rotate_every_two(t) * sin_p


@functools.lru_cache(maxsize=None)
def _attn_caches(dn, window, N):
    g = _gen(12000 + window + N)
    B, H = ATTN_B, ATTN_H
    return _randn(g, B, H, N, 64), _randn(g, B, H, N, 64)


@functools.lru_cache(maxsize=None)
def attn_inputs(case):
    dn, kind, window, N, pos = case
    dtype = _dt(dn)
    B, H = ATTN_B, ATTN_H
    g = _gen(12100 + 3 * window + N + 17 * pos)
    sin, cos = rope_tables(N)
    qkv = _randn(g, B, 3, H, 64)
    k0, v0 = (t.clone() for t in _attn_caches(dn, window, N))
    start, nrows = band(window, pos)
    if kind != "rand":
        qkv[:, 0] *= 6.0
        q_rot = _rot(qkv[:, 0].to(dtype).float(), sin[pos], cos[pos])
        k0[:, :, start if kind == "peak_first" else pos - 1] = PEAK * q_rot
    for c in (k0, v0):
        c[:, :, pos:] = NAN       # rows after pos, and row pos itself
        c[:, :, :start] = NAN     # rows before the band
    return dict(qkv=qkv.reshape(B, 3 * H * 64).to(dtype), sin=sin, cos=cos,
                pos=pos, k_cache=k0.to(dtype), v_cache=v0.to(dtype),
                window=window)


def attn_explicit(qkv, sin, cos, pos, k_cache, v_cache, window, rnd=ident,
                  mutant=None):
    """decode_attn_body.h in formulas, with its 32 groups / 4 waves; returns
    out (B, H, 64) and the k and v rows written at ``pos``"""
    B, H, N, _ = k_cache.shape
    dt = qkv.dtype
    sp, cp = sin[pos].to(dt), cos[pos].to(dt)
    q, k, v = qkv.reshape(B, 3, H, 64).unbind(1)
    q, k = rnd(_rot(q, sp, cp)), rnd(_rot(k, sp, cp))
    v = rnd(v) if mutant == "v_not_rotated" else rnd(_rot(v, sp, cp))
    scale = 1.0 if mutant == "no_scale" else 0.125
    ninf = torch.full((B, H, GROUPS), -math.inf, dtype=dt)

    m, l = ninf.clone(), torch.zeros(B, H, GROUPS, dtype=dt)
    acc = torch.zeros(B, H, GROUPS, 64, dtype=dt)
    s0 = (q * k).sum(-1) * scale
    lookback = pos < window
    if mutant == "no_zero_lookback":
        lookback = False
    elif mutant == "zero_lookback_kept":
        lookback = pos < 2 * window
    if mutant == "current_row_left_out":
        if lookback:
            m[:, :, 0], l[:, :, 0] = 0.0, float(window)
    elif lookback:
        nzero = window - 1 if mutant == "zero_count_minus1" else window
        m0 = s0.clamp_min(0.0)
        e = torch.exp(s0 - m0)
        m[:, :, 0] = m0
        l[:, :, 0] = e + nzero * torch.exp(-m0)
        acc[:, :, 0] = e.unsqueeze(-1) * v
    else:
        m[:, :, 0], l[:, :, 0], acc[:, :, 0] = s0, 1.0, v

    w0 = (pos // window) * window
    start = w0 if mutant == "band_starts_at_w0" else max(w0 - window, 0)
    nrows = pos - start
    if mutant == "last_row_dropped":
        nrows -= 1
    grp = torch.arange(GROUPS)
    for r0 in range(0, nrows, GROUPS):
        r = r0 + grp
        has = (r < nrows).reshape(1, 1, GROUPS)
        rows = start + r.clamp_max(nrows - 1)     # a live row where has not
        kk, vv = k_cache[:, :, rows], v_cache[:, :, rows]
        s = (q.unsqueeze(2) * kk).sum(-1) * scale
        mn = torch.maximum(m, s)
        a = torch.exp(m - mn)                     # 0 on a group's first row
        e = torch.exp(s - mn)
        l = torch.where(has, l * a + e, l)
        acc = torch.where(has.unsqueeze(-1),
                          acc * a.unsqueeze(-1) + e.unsqueeze(-1) * vv, acc)
        m = torch.where(has, mn, m)

    def join(m, l, acc, size):
        """``size`` neighbours under their common maximum"""
        shape = m.shape[:2] + (-1, size)
        mg = m.reshape(shape)
        top = mg.amax(-1, keepdim=True)
        wgt = torch.exp(mg - top)                 # nan where both are -inf
        if mutant != "empty_unguarded":
            wgt = torch.where(mg == -math.inf, torch.zeros_like(wgt), wgt)
        return (top.squeeze(-1), (l.reshape(shape) * wgt).sum(-1),
                (acc.reshape(shape + (64,)) * wgt.unsqueeze(-1)).sum(-2))

    m, l, acc = join(m, l, acc, 8)                # the 8 groups of a wave
    m, l, acc = join(m, l, acc, 4)                # the 4 waves
    out = rnd(acc.squeeze(2) * (1.0 / l))
    res = dict(out=out, k=k, v=v)
    if mutant == "head_batch_swapped":
        # block i takes (i % B, i // B) for (i // H, i % H)
        i = torch.arange(B * H)
        perm = (i % B) * H + i // B
        res = {n: t.reshape(B * H, 64)[perm].reshape(B, H, 64)
               for n, t in res.items()}
    return res


def _rand(c):
    return c[1] == "rand"


def _nrows(c):
    return band(c[2], c[4])[1]


ATTN_MUTANTS = {
    # at position 0 the rotation is the identity
    "v_not_rotated": lambda c: c[4] >= 1,
    # a one-hot softmax stays one-hot at eight times the logits
    "no_scale": _rand,
    # the lookback window is skipped: from the third window on; a peak at
    # row pos - 1 is in the current window and hides the loss
    "band_starts_at_w0": lambda c: c[4] >= 2 * c[2] and c[1] != "peak_last",
    # the zero keys only weigh where no logit towers over 0
    "no_zero_lookback": lambda c: _rand(c) and c[4] < c[2],
    "zero_lookback_kept": lambda c: _rand(c) and c[2] <= c[4] < 2 * c[2],
    # one zero key of ``window``: 1 / (64 + a few) of the mass, about
    # 1.5 % of a row at window 64 with at most 8 cached rows; beyond that
    # the bf16 bound no longer sees it
    "zero_count_minus1": lambda c: _rand(c) and c[4] < c[2] and (
        c[0] == "fp32" or (c[2] == 64 and _nrows(c) <= 8)),
    "current_row_left_out": lambda c: _rand(c) and _nrows(c) <= 8,
    # the newest cached row: the peak itself in the peak_last cases
    "last_row_dropped": lambda c: c[1] != "peak_first" and
    1 <= _nrows(c) <= 33,
    "head_batch_swapped": lambda c: True,
    # the kernel gives a group without rows the weight 0 explicitly. Giving
    # it the weight 1 instead computes the same thing, since its l and acc
    # are 0; what the guard keeps out is exp(-inf - -inf) = nan of a WAVE
    # without rows, so the mutant is the unguarded exp, and it applies where
    # wave 3 (groups 24..31) is empty
    "empty_unguarded": lambda c: _nrows(c) <= 24,
}


def attn_emulate(case, mutant=None, dt=F32):
    inp = {k: (_to(v, dt) if torch.is_tensor(v) else v)
           for k, v in attn_inputs(case).items()}
    return attn_explicit(**inp, rnd=_rnd(case[0], dt), mutant=mutant)


@functools.lru_cache(maxsize=None)
def attn_oracle(case):
    inp = attn_inputs(case)
    B, H, pos = ATTN_B, ATTN_H, inp["pos"]
    kc, vc = inp["k_cache"].to(F64).clone(), inp["v_cache"].to(F64).clone()
    out = R.decode_attention(inp["qkv"].to(F64), inp["sin"], inp["cos"],
                             torch.tensor(pos), kc, vc, inp["window"])
    return dict(out=out.reshape(B, H, 64), k=kc[:, :, pos].clone(),
                v=vc[:, :, pos].clone())


def attn_errors(got, want, case):
    """out in both dtypes; the written rows by ``row_err`` in fp32. In bf16
    they are held as rope_qkv is: ``kv_ulp``, the largest distance in bf16
    steps from the correctly rounded fp64 rotation, with the bound 1"""
    errs = dict(out=row_err(got["out"], want["out"]))
    if case[0] == "fp32":
        errs["k"] = row_err(got["k"], want["k"])
        errs["v"] = row_err(got["v"], want["v"])
    else:
        errs["kv_ulp"] = float(attn_row_ulps(got, want))
    return errs


def attn_row_ulps(got, want):
    """bf16 steps between the written k / v rows and the rounded oracle;
    a non-finite row is infinitely far"""
    if not all(torch.isfinite(got[n]).all() for n in ("k", "v")):
        return math.inf
    return max(bf16_ulp_dist(got[n].to(BF16), want[n]) for n in ("k", "v"))


# ---------------------------------------------------------------------------
# dec_sgu
# ---------------------------------------------------------------------------

SGU_B = 2
# (N, d2): one tile; N not a power of two with three tiles; 33 tiles and
# 264 chunks a row, so that threads 0..7 of the statistics loop own two
SGU_SHAPES = ((256, 64), (192, 192), (256, 2112))


def sgu_positions(N):
    return (0, 1, 2, 31, 32, 33, 127, 128, 129, N - 1)


def sgu_cases(dtype):
    """(dtype name, N, d2, pos)"""
    return [(dname(dtype), N, d2, pos)
            for N, d2 in SGU_SHAPES for pos in sgu_positions(N)]


@functools.lru_cache(maxsize=None)
def _sgu_shared(dn, N, d2):
    """the weights and the history of a shape, shared by its positions"""
    dtype = _dt(dn)
    g = _gen(13000 + N + d2)
    return dict(g=(1 + 0.25 * _randn(g, d2)).to(dtype),
                w=(_randn(g, N, N) / 16).to(dtype),
                bias=_randn(g, N, 1).to(dtype),
                hist=_randn(g, SGU_B, N, d2).to(dtype))


@functools.lru_cache(maxsize=None)
def sgu_inputs(case):
    """the xa half is five times as loud as the gate half and off centre:
    statistics taken from it are far from the gate's"""
    dn, N, d2, pos = case
    sh = _sgu_shared(dn, N, d2)
    g = _gen(13100 + N + d2 + 19 * pos)
    h = _randn(g, SGU_B, 2 * d2)
    h[:, :d2] = 5 * h[:, :d2] + 3
    hist = sh["hist"].clone()
    hist[:, pos:] = NAN           # rows after pos, and row pos itself
    return dict(h=h.to(_dt(dn)), g=sh["g"], hist=hist, w=sh["w"],
                bias=sh["bias"], pos=pos)


def sgu_explicit(h, g, hist, w, bias, pos, rnd=ident, mutant=None):
    """decode_sgu_body.h in formulas; returns out and the history row
    written at ``pos``"""
    d2 = g.shape[0]
    xa, gate = h[:, :d2], h[:, d2:]
    st = xa if mutant == "stats_from_xa" else gate
    mu = st.mean(-1, keepdim=True)
    var = ((st - mu) ** 2).mean(-1, keepdim=True)
    gl = rnd((gate - mu) * torch.rsqrt(var + EPS) * g)
    n = pos - 1 if mutant == "last_row_dropped" else pos
    n = max(n, 0)
    wrow = w[:n, pos] if mutant == "w_transposed" else w[pos, :n]
    t = torch.einsum("n,bnd->bd", wrow, hist[:, :n])
    if mutant != "no_pos_term":
        t = t + w[pos, pos] * gl
    if mutant != "no_bias":
        t = t + bias[0 if mutant == "bias_at_0" else pos]
    return dict(out=rnd(xa * t), hist=gl)


# a mutant that loses one term is as visible as that term is large: it
# applies where the weight or bias it loses is at least half its standard
# deviation (1/16 for w, 1 for the bias)
SGU_W_MIN, SGU_BIAS_MIN = 1.0 / 32, 0.5


def _w_at(c, i, j):
    return abs(float(_sgu_shared(*c[:3])["w"][i, j]))


def _bias_at(c, i):
    return float(_sgu_shared(*c[:3])["bias"][i, 0])


SGU_MUTANTS = {
    "no_pos_term": lambda c: _w_at(c, c[3], c[3]) >= SGU_W_MIN,
    "no_bias": lambda c: abs(_bias_at(c, c[3])) >= SGU_BIAS_MIN,
    "last_row_dropped": lambda c: c[3] >= 1 and
    _w_at(c, c[3], c[3] - 1) >= SGU_W_MIN,
    # w[n, pos] for w[pos, n]: the diagonal term is the same in both, so it
    # is held where there are 31 rows or more below pos
    "w_transposed": lambda c: c[3] >= 31,
    "bias_at_0": lambda c: c[3] >= 1 and
    abs(_bias_at(c, c[3]) - _bias_at(c, 0)) >= SGU_BIAS_MIN,
    "stats_from_xa": lambda c: True,
}


def sgu_emulate(case, mutant=None, dt=F32):
    inp = {k: (_to(v, dt) if torch.is_tensor(v) else v)
           for k, v in sgu_inputs(case).items()}
    return sgu_explicit(**inp, rnd=_rnd(case[0], dt), mutant=mutant)


@functools.lru_cache(maxsize=None)
def sgu_oracle(case):
    inp = sgu_inputs(case)
    pos = inp["pos"]
    hist = inp["hist"].to(F64).clone()
    out = R.decode_sgu(inp["h"].to(F64), inp["g"].to(F64), hist,
                       inp["w"].to(F64), inp["bias"].to(F64),
                       torch.tensor(pos), EPS)
    return dict(out=out, hist=hist[:, pos].clone())


def sgu_errors(got, want, case=None):
    return {k: row_err(got[k], want[k]) for k in ("out", "hist")}


# ---------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------

FAMILIES = ("dec_ln", "dec_ln_res", "dec_attn", "dec_sgu")
MUTANTS = {"dec_ln": LN_MUTANTS, "dec_ln_res": LN_MUTANTS,
           "dec_attn": ATTN_MUTANTS, "dec_sgu": SGU_MUTANTS}


def family_cases(family, dn):
    dtype = _dt(dn)
    if family in ("dec_ln", "dec_ln_res"):
        return [c for c in ln_cases(dtype) if ln_family(c) == family]
    return attn_cases(dtype) if family == "dec_attn" else sgu_cases(dtype)


def _parts(family):
    """(emulate, oracle, errors) of a family"""
    if family in ("dec_ln", "dec_ln_res"):
        return ln_emulate, ln_oracle, ln_errors
    if family == "dec_attn":
        return attn_emulate, attn_oracle, attn_errors
    return sgu_emulate, sgu_oracle, sgu_errors


def errors(family, case, got=None, mutant=None):
    """{output: row_err against the oracle} of ``got``, or of the emulation
    (with ``mutant``) where none is given"""
    emulate, oracle, errs = _parts(family)
    if got is None:
        got = emulate(case, mutant)
    return errs(got, oracle(case), case)


@functools.lru_cache(maxsize=None)
def bounds(family, dn):
    """{output: (emulation error, bound)}, worst case over the family"""
    worst = {}
    for c in family_cases(family, dn):
        for k, v in errors(family, c).items():
            worst[k] = max(worst.get(k, 0.0), v)
    return {k: (v, 1.0 if k == "kv_ulp" else MARGIN * v)
            for k, v in worst.items()}


def misses(family, dn, errs):
    """the outputs of ``errs`` that are over their bound"""
    b = bounds(family, dn)
    return [(k, v, b[k][1]) for k, v in errs.items() if not v <= b[k][1]]
