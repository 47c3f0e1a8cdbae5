"""GPU: the decode linear kernel (progen_amd/ops/hip/decode_linear.hip)
against an fp64 oracle by the method of tests/KERNEL_TOLERANCES.md, the
fused decode step with ``fused_linear=True`` against the HIP full forward,
and its hipGraph capture.

Three computations of every case, on the dtype-rounded inputs:

  oracle     ``reference.decode_linear`` in fp64;
  emulation  the same formula in fp32, summed in the kernel's own order: a
             lane's chain over its 16-element chunks (vec path; on the mfma
             path one instruction's 32 exact products are one fp32 sum added
             to the accumulator — the order inside the instruction is the
             hardware's), the four lanes of a row as (g0 + g1) + (g2 + g3),
             the waves in wave order; bias, then the activation with
             ``fast_tanh`` as ``kernel_oracle.gelu_tanh_parts(fast=True)``
             models it; rounded to bf16 only at the store;
  mutants    the emulation with one defect: bias dropped, GLU halves
             swapped, the last K-step skipped.

The bound of a (act, dtype) family is MARGIN x the emulation's ``row_err``
against the oracle, worst case over the family's cases, computed here. The
CPU checks of this file show that the emulation passes it and that every
mutant misses it.

Cases: B on both sides of every batch at which the kernel changes path or
tile (4/5 vec -> mfma, 16/17 one -> two batch tiles; fp32 takes 4-row
chunks of the vec path), K of one step, an odd number of steps, and more
passes of the K split than one (6144 only with the narrowest N), N of one
tile, three, five and sixteen tiles — every N the contract admits is whole
16-column tiles, so there is no partial one — and both sides of the two
tile counts (256, 512) at which the launcher changes the waves per
workgroup. No test launches outside [1, 32] rows.
"""

import functools

import pytest
import torch

from kernel_oracle import (BF16, F32, F64, MARGIN, dname, gelu_tanh_parts,
                           rounder, row_err)
from progen_amd.ops import functional as OF, reference as R

pytestmark = pytest.mark.gpu

ACTS = ("none", "gelu", "glu")
DTYPES = (BF16, F32)
NAN = float("nan")
VEC_MAX_B = 4      # DEC_LINEAR_VEC_MAX_B of decode_linear_kernels.h


def dev():
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------

def cases(dn, act):
    """(dtype name, act, bias, B, K, N) with N the weight rows"""
    m = 2 if act == "glu" else 1
    out = []
    for bias in (True, False):
        out += [(dn, act, bias, B, 192, 48 * m)
                for B in (1, 2, 4, 5, 16, 17, 32)]
        out += [(dn, act, bias, B, K, N * m)
                for B in (2, 5, 17)
                for K, N in ((64, 256), (1536, 256), (6144, 16))]
        out += [(dn, act, bias, B, 64, N * m)
                for B in (1, 5) for N in (16, 80)]
    # the launcher's wave-count thresholds: 255/256 and 511/512 tiles
    out += [(dn, act, True, B, 64, 16 * tiles * m)
            for B in (2, 5) for tiles in (255, 256, 511, 512)]
    return out


@functools.lru_cache(maxsize=None)
def inputs(case):
    """x ~ N(0, 1), w ~ N(0, 1/K): pre-activations of order one, so that
    the bias (0.5 N(0, 1)) and each half of a GLU carry weight"""
    dn, act, bias, B, K, N = case
    dtype = {"bf16": BF16, "fp32": F32}[dn]
    g = torch.Generator().manual_seed(9000 + 7 * B + K + 3 * N)
    x = torch.randn(B, K, generator=g, dtype=F32).to(dtype)
    w = (torch.randn(N, K, generator=g, dtype=F32) * K ** -0.5).to(dtype)
    b = (0.5 * torch.randn(N, generator=g, dtype=F32)).to(dtype) \
        if bias else None
    return x, w, b


@functools.lru_cache(maxsize=None)
def oracle(case):
    x, w, b = inputs(case)
    return R.decode_linear(x.to(F64), w.to(F64),
                           None if b is None else b.to(F64), case[1])


# ---------------------------------------------------------------------------
# emulation
# ---------------------------------------------------------------------------

def waves_for(tiles):
    nw = 4
    while nw < 16 and tiles * nw < 2048:
        nw *= 2
    return nw


def emulate(case, mutant=None):
    dn, act, _, B, K, N = case
    dtype = {"bf16": BF16, "fp32": F32}[dn]
    x, w, b = (None if t is None else t.to(F32) for t in inputs(case))
    glu = act == "glu"
    mfma = dtype == BF16 and B > VEC_MAX_B
    nw = waves_for((N // 2 if glu else N) // 16)
    if mfma and glu and B > 16:
        nw = min(nw, 8)
    ksteps = K // 64
    if mutant == "last_kstep_skipped":
        x = x.clone()
        x[:, K - 64:] = 0
    # wave v takes steps v, v + nw, ...; lane group g the 16 elements at
    # 16 g of a step: (iteration, wave, group, element)
    iters = -(-ksteps // nw)
    pad = iters * nw * 64 - K
    xr = torch.nn.functional.pad(x, (0, pad)).view(B, 1, iters, nw, 4, 16)
    wr = torch.nn.functional.pad(w, (0, pad)).view(1, N, iters, nw, 4, 16)
    if mfma:
        acc = torch.zeros(B, N, nw, dtype=F32)
        for it in range(iters):
            for s in range(2):
                sl = slice(8 * s, 8 * s + 8)
                p = xr[:, :, it, :, :, sl] * wr[:, :, it, :, :, sl]
                acc = acc + p.sum(dim=(-1, -2))
    else:
        acc = torch.zeros(B, N, nw, 4, dtype=F32)
        for it in range(iters):
            for j in range(16):
                acc = acc + xr[:, :, it, :, :, j] * wr[:, :, it, :, :, j]
        acc = (acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])
    h = torch.zeros(B, N, dtype=F32)
    for v in range(nw):
        h = h + acc[:, :, v]
    if b is not None and mutant != "bias_dropped":
        h = h + b
    if glu:
        a, g = h.chunk(2, dim=-1)
        if mutant == "halves_swapped":
            a, g = g, a
        y = a * gelu_tanh_parts(g, fast=True)[0]
    elif act == "gelu":
        y = gelu_tanh_parts(h, fast=True)[0]
    else:
        y = h
    return rounder(dtype)(y)


MUTANTS = {"bias_dropped": lambda c: c[2],
           "halves_swapped": lambda c: c[1] == "glu",
           "last_kstep_skipped": lambda c: True}


@functools.lru_cache(maxsize=None)
def bound(dn, act):
    """(emulation error, bound) of the family"""
    emu = max(row_err(emulate(c), oracle(c)) for c in cases(dn, act))
    return emu, MARGIN * emu


# ---------------------------------------------------------------------------
# CPU: the comparator tells the emulation from its mutants
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
def test_emulation_passes_and_mutants_miss_the_bound(dtype, act):
    dn = dname(dtype)
    emu, bnd = bound(dn, act)
    print(f"KTOL|dec_linear_{act}|out|{dn}|{emu:.3e}|{bnd:.3e}|emulation")
    assert 0 < emu <= bnd
    # the storage format sets the scale: a few bf16 / fp32 roundings
    assert bnd < (2e-2 if dtype == BF16 else 1e-5)
    for name, applies in MUTANTS.items():
        hit = [c for c in cases(dn, act) if applies(c)]
        if name == "halves_swapped" and act != "glu":
            assert not hit
            continue
        assert hit, name
        for c in hit:
            err = row_err(emulate(c, mutant=name), oracle(c))
            assert err > bnd, (name, c, err, bnd)


# ---------------------------------------------------------------------------
# GPU: the kernel
# ---------------------------------------------------------------------------

def run_kernel(x, w, b, act):
    assert OF.decode_linear_supported(x.shape[0], x.shape[1], w.shape[0],
                                      act, x.dtype)
    return OF.decode_linear(x.to(dev()), w.to(dev()),
                            None if b is None else b.to(dev()), act)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
def test_kernel_within_the_bound(dtype, act, monkeypatch):
    # the kernel's own range, whatever the routing limit is set to
    monkeypatch.setattr(OF, "DEC_LINEAR_MAX_B", OF.DEC_LINEAR_KERNEL_MAX_B)
    dn = dname(dtype)
    emu, bnd = bound(dn, act)
    missed, worst = [], 0.0
    for c in cases(dn, act):
        x, w, b = inputs(c)
        got = run_kernel(x, w, b, act)
        want = oracle(c)
        assert got.dtype == dtype and got.shape == want.shape, c
        err = row_err(got, want)
        worst = max(worst, err)
        if not err <= bnd:
            missed.append((c, err))
    print(f"KTOL|dec_linear_{act}|out|{dn}|{emu:.3e}|{bnd:.3e}|{worst:.3e}|"
          f"kernel")
    assert not missed, (bnd, missed)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
def test_nan_rows_do_not_cross_batch_rows(dtype, act, monkeypatch):
    """Rows 0..2 of a 16-row x whose other rows are NaN: with all 16 rows
    launched (bf16: one mfma batch tile; fp32: four vec chunks, the first
    of them mixed) and with only the three rows launched, which the kernel
    must not read past."""
    monkeypatch.setattr(OF, "DEC_LINEAR_MAX_B", OF.DEC_LINEAR_KERNEL_MAX_B)
    dn = dname(dtype)
    _, bnd = bound(dn, act)
    c = (dn, act, True, 3, 192, 96 if act == "glu" else 48)
    x, w, b = inputs(c)
    want = R.decode_linear(x.to(F64), w.to(F64), b.to(F64), act)
    x16 = torch.full((16, x.shape[1]), NAN, dtype=dtype)
    x16[:3] = x
    x16 = x16.to(dev())
    for rows in (16, 3):
        got = OF.decode_linear(x16[:rows], w.to(dev()), b.to(dev()), act)
        assert got.shape[0] == rows
        assert torch.isfinite(got[:3]).all(), rows
        assert row_err(got[:3], want) <= bnd, rows
        if rows == 16:
            assert torch.isnan(got[3:]).all()


# ---------------------------------------------------------------------------
# the whole step
# ---------------------------------------------------------------------------

def rel_err(got, want):
    got = got.float().cpu()
    want = want.float().cpu()
    denom = want.abs().max().clamp_min(1e-6)
    return ((got - want).abs().max() / denom).item()


def _count_kernel_calls(monkeypatch):
    """every decode_linear call of the step must route to the kernel"""
    routed = []
    real = OF.decode_linear_supported
    monkeypatch.setattr(OF, "decode_linear_supported",
                        lambda *a: routed.append(real(*a)) or routed[-1])
    return routed


def test_fused_linear_decode_matches_hip_forward(monkeypatch):
    """The model and bound of
    test_gpu_decode_fused.py::test_fused_decode_matches_hip_forward."""
    from progen_amd import ProGenBase, ProGenConfig
    from progen_amd.decode import DecodeCache, forward_step_fused
    routed = _count_kernel_calls(monkeypatch)
    cfg = ProGenConfig(num_tokens=256, dim=128, seq_len=256, depth=3,
                       window_size=64, global_mlp_depth=1, heads=2, dim_head=64)
    torch.manual_seed(5)
    m = ProGenBase(cfg).to(device=dev(), dtype=torch.bfloat16)
    m.rotary_sin = m.rotary_sin.float()
    m.rotary_cos = m.rotary_cos.float()

    seq = torch.randint(1, 256, (256,), device=dev())
    with torch.no_grad():
        full = m(seq.unsqueeze(0))[0].float()

    cache = DecodeCache(m, batch=1)
    pos = torch.zeros((), dtype=torch.long, device=dev())
    rows = []
    for p in range(256):
        rows.append(forward_step_fused(m, seq[p:p + 1], cache, pos,
                                       fused_linear=True))
        pos += 1
    inc = torch.cat(rows, dim=0).float()
    assert routed and all(routed)
    assert rel_err(inc, full) < 6e-2


def _graph_model():
    # the model of tests/test_gpu_decode_graph.py
    from progen_amd import ProGenBase, ProGenConfig
    cfg = ProGenConfig(num_tokens=256, dim=256, depth=3, heads=4,
                       dim_head=64, window_size=64, seq_len=256,
                       ff_glu=False, global_mlp_depth=1)
    torch.manual_seed(3)
    m = ProGenBase(cfg).to(device="cuda", dtype=torch.bfloat16).eval()
    m.rotary_sin = m.rotary_sin.float()
    m.rotary_cos = m.rotary_cos.float()
    return m


def _prefill(m, prime):
    from progen_amd.decode import DecodeCache, forward_step_fused
    cache = DecodeCache(m, batch=1)
    pos = torch.zeros((), dtype=torch.long, device="cuda")
    logits = None
    for p in range(len(prime)):
        logits = forward_step_fused(m, prime[p:p + 1].cuda(), cache, pos,
                                    fused_linear=True)
        pos += 1
    return cache, pos, logits.cpu().float().argmax(dim=-1)


def test_graphed_fused_linear_decode_matches_uncaptured(monkeypatch):
    """No atomics and a fixed summation order: a replay reproduces the
    uncaptured step bit for bit, so greedy tokens are equal."""
    from progen_amd.decode import GraphedDecodeStep, forward_step_fused
    routed = _count_kernel_calls(monkeypatch)
    m = _graph_model()
    torch.manual_seed(11)
    prime = torch.randint(1, 256, (17,))
    n = 40

    cache, pos, tok = _prefill(m, prime)
    want = []
    for _ in range(n):
        want.append(int(tok))
        logits = forward_step_fused(m, tok.cuda(), cache, pos,
                                    fused_linear=True)
        pos += 1
        tok = logits.cpu().float().argmax(dim=-1)

    cache, pos, tok = _prefill(m, prime)
    g = GraphedDecodeStep(m, cache, start_pos=len(prime), fused=True,
                          fused_linear=True)
    got = []
    for _ in range(n):
        got.append(int(tok))
        tok = g.step(tok).cpu().float().argmax(dim=-1)
    assert routed and all(routed)
    assert got == want, (got, want)
    assert int(g.pos_dev) == len(prime) + n == cache.pos
