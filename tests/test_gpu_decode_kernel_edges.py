"""GPU: the three decode-step kernels (progen_amd/ops/hip/decode_*_body.h)
at their branch points against the fp64 oracle, and the whole fused step
against an fp64 forward.

The cases, oracles and bounds are those of tests/decode_oracle.py, whose
bounds tests/test_decode_oracle.py shows to reject every listed mutant;
the method is that of tests/KERNEL_TOLERANCES.md. One test per kernel and
dtype loops over the kernel's cases: a launch is microseconds. For each
case it holds

  - every output to its ``row_err`` bound, the row a step writes into a
    cache included (bf16 k / v rows: within one bf16 step of the correctly
    rounded fp64 rotation);
  - every other row of a cache, history or prev, and every input that is
    not updated, to the bits it had;
  - the output to be finite although every row a step must not read holds
    NaN.

and prints the worst figure of each output as a ``KTOL|...`` line in the
format of ``kernel_oracle.check``. No launch uses a position outside
[0, N).

The whole step: logits of 256 fused steps at batch 3 and of the HIP full
forward, each against an fp64 CPU forward on the same bf16-rounded weights.
The full forward is another, oracle-tested path; the fused steps may be
twice as far from the truth as it is, the margin for accumulation order.
"""

import copy

import pytest
import torch

import decode_oracle as O
from kernel_oracle import BF16, F32, dname
from progen_amd.ops import dispatch, functional as OF

pytestmark = pytest.mark.gpu

DTYPES = (BF16, F32)


def dev():
    return torch.device("cuda:0")


def bits(x):
    """Raw storage bits, so that NaN rows compare equal to themselves."""
    x = x.detach().cpu().contiguous()
    return x.view(torch.int16 if x.dtype == BF16 else torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def gpu(t):
    return None if t is None else t.to(dev())


def routed_to_hip(op):
    """the debug switches that send an op to its torch reference are off:
    what is measured is the kernel"""
    return dispatch.use_hip(torch.empty(1, device=dev()), op)


class Worst:
    """worst measured figure of each output of a family, with its case"""

    def __init__(self, family, dn):
        self.family, self.dn = family, dn
        self.worst, self.missed = {}, []

    def add(self, case, errs):
        for k, v in errs.items():
            if not v <= self.worst.get(k, (-1.0, None))[0]:
                self.worst[k] = (v, case)
        self.missed += [(case, m) for m in O.misses(self.family, self.dn, errs)]

    def report(self):
        b = O.bounds(self.family, self.dn)
        for k, (v, case) in self.worst.items():
            emu, bound = b[k]
            print(f"KTOL|{self.family}|{k}|{self.dn}|{emu:.3e}|{bound:.3e}|"
                  f"{v:.3e}|{case}")
        assert not self.missed, self.missed


# ---------------------------------------------------------------------------
# dec_ln_shift
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
def test_dec_ln_shift_within_the_bounds(dtype):
    assert routed_to_hip("dec_ln")
    dn = dname(dtype)
    fams = {f: Worst(f, dn) for f in ("dec_ln", "dec_ln_res")}
    for case in O.ln_cases(dtype):
        inp = O.ln_inputs(case)
        _, B, D, shift, res, prev = case
        h, r, g, pv = (gpu(inp[k]) for k in ("h", "res", "g", "prev"))
        h, pv = h.clone(), None if pv is None else pv.clone()
        y = OF.decode_ln_shift(h, r, g, pv, shift=shift)
        assert y.dtype == dtype and y.shape == (B, D), case
        fams[O.ln_family(case)].add(
            case, O.ln_errors(dict(y=y, h=h, prev=pv), O.ln_oracle(case),
                              case))
        assert same(g, inp["g"]), case
        if res:
            assert same(r, inp["res"]), case
        else:
            assert same(h, inp["h"]), case      # nothing added: not rewritten
        if shift:
            # the shifted half is a copy of the previous row, bit for bit
            assert same(y[:, :D // 2], inp["prev"][:, :D // 2]), case
        if prev:
            # prev is the whole LN row: its other half is what y carries
            assert same(pv[:, D // 2:], y[:, D // 2:]), case
    for w in fams.values():
        w.report()


# ---------------------------------------------------------------------------
# dec_attn
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
def test_dec_attn_within_the_bounds(dtype):
    assert routed_to_hip("dec_attn")
    dn = dname(dtype)
    worst = Worst("dec_attn", dn)
    B, H = O.ATTN_B, O.ATTN_H
    tables = {}
    for case in O.attn_cases(dtype):
        inp = O.attn_inputs(case)
        _, _, window, N, p = case
        if N not in tables:
            tables[N] = gpu(inp["sin"]), gpu(inp["cos"])
        sin, cos = tables[N]
        qkv, k_d, v_d = (gpu(inp[k]) for k in ("qkv", "k_cache", "v_cache"))
        pos = torch.tensor(p, dtype=torch.long, device=dev())
        out = OF.decode_attention(qkv, sin, cos, pos, k_d, v_d, window)
        assert out.dtype == dtype and out.shape == (B, H * 64), case
        assert torch.isfinite(out).all(), case
        assert int(pos) == p and same(qkv, inp["qkv"]), case
        others = [i for i in range(N) if i != p]
        for after, before in ((k_d, inp["k_cache"]), (v_d, inp["v_cache"])):
            assert same(after[:, :, others], before[:, :, others]), case
        got = dict(out=out.reshape(B, H, 64), k=k_d[:, :, p], v=v_d[:, :, p])
        worst.add(case, O.attn_errors(got, O.attn_oracle(case), case))
    worst.report()


# ---------------------------------------------------------------------------
# dec_sgu
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
def test_dec_sgu_within_the_bounds(dtype):
    assert routed_to_hip("dec_sgu")
    dn = dname(dtype)
    worst = Worst("dec_sgu", dn)
    shared = {}
    for case in O.sgu_cases(dtype):
        inp = O.sgu_inputs(case)
        _, N, d2, p = case
        if (N, d2) not in shared:
            shared[(N, d2)] = tuple(gpu(inp[k]) for k in ("g", "w", "bias"))
        g, w, bias = shared[(N, d2)]
        h, hist = gpu(inp["h"]), gpu(inp["hist"])
        pos = torch.tensor(p, dtype=torch.long, device=dev())
        out = OF.decode_sgu(h, g, hist, w, bias, pos)
        assert out.dtype == dtype and out.shape == (O.SGU_B, d2), case
        assert torch.isfinite(out).all(), case
        assert int(pos) == p and same(h, inp["h"]), case
        assert same(g, inp["g"]) and same(w, inp["w"]) and \
            same(bias, inp["bias"]), case
        others = [i for i in range(N) if i != p]
        assert same(hist[:, others], inp["hist"][:, others]), case
        worst.add(case, O.sgu_errors(dict(out=out, hist=hist[:, p]),
                                     O.sgu_oracle(case)))
    worst.report()


# ---------------------------------------------------------------------------
# the whole fused step against fp64
# ---------------------------------------------------------------------------

def rel_err(got, want):
    # tests/test_gpu_prefill.py
    got = got.double().cpu()
    want = want.double().cpu()
    denom = want.abs().max().clamp_min(1e-6)
    return ((got - want).abs().max() / denom).item()


def test_fused_steps_are_as_close_to_fp64_as_the_full_forward():
    """The model of
    test_gpu_decode_fused.py::test_fused_decode_matches_hip_forward, at
    batch 3."""
    from progen_amd import ProGenBase, ProGenConfig
    from progen_amd.decode import DecodeCache, forward_step_fused
    B, N = 3, 256
    cfg = ProGenConfig(num_tokens=256, dim=128, seq_len=N, depth=3,
                       window_size=64, global_mlp_depth=1, heads=2, dim_head=64)
    torch.manual_seed(5)
    m = ProGenBase(cfg).to(device=dev(), dtype=BF16).eval()
    m.rotary_sin = m.rotary_sin.float()
    m.rotary_cos = m.rotary_cos.float()
    # the same bf16-rounded weights on the CPU, in fp64
    m64 = copy.deepcopy(m).to(device="cpu", dtype=torch.float64)
    m64.rotary_sin = m64.rotary_sin.float()
    m64.rotary_cos = m64.rotary_cos.float()

    seq = torch.randint(1, 256, (B, N),
                        generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        want = m64(seq)
        full = m(seq.to(dev()))
    e_full = rel_err(full, want)
    assert want.shape == full.shape == (B, N, 256)

    tok = seq.to(dev())
    for fused_linear in (False, True):
        cache = DecodeCache(m, batch=B)
        pos = torch.zeros((), dtype=torch.long, device=dev())
        rows = []
        for p in range(N):
            rows.append(forward_step_fused(m, tok[:, p].contiguous(), cache,
                                           pos, fused_linear=fused_linear))
            pos += 1
        e_steps = rel_err(torch.stack(rows, dim=1), want)
        print(f"STEP64|B={B}|N={N}|fused_linear={fused_linear}|"
              f"steps={e_steps:.3e}|full_forward={e_full:.3e}")
        assert e_steps <= 2 * e_full, (fused_linear, e_steps, e_full)
