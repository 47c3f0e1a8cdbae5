"""GPU: the prefill kernels (progen_amd._C_prefill) and ``decode.prefill``
on them.

The kernels are held to what they share with existing ones: the rotation to
``rope_qkv``'s bits, the cache rows to the bits of the full-sequence output,
the gate LN to the fp64 oracle within kernel_oracle's ``ln`` bound, rows
>= P to the bits they had. The whole prefill is compared with P calls of
``forward_step_fused``, both against an fp64 CPU ``forward_step`` on the
same bf16-rounded weights; the step loops run once per batch size.
Every figure is printed as a ``PREFILL|...`` line before it is asserted.
"""

import copy
import functools

import pytest
import torch

import kernel_oracle as K
from progen_amd import decode
from progen_amd.ops import dispatch, reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
NAN = float("nan")


def rel_err(got, want):
    got = got.double().cpu()
    want = want.double().cpu()
    denom = want.abs().max().clamp_min(1e-6)
    return ((got - want).abs().max() / denom).item()


def bits(t):
    return t.contiguous().view(torch.int16).cpu()


# ---------------------------------------------------------------------------
# prefill_rope_kv
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("Np", [64, 256])
@pytest.mark.parametrize("P", [1, 63, 64, "Np"])
def test_prefill_rope_kv(Np, P):
    B, H, Nc = 2, 2, 256
    P = Np if P == "Np" else P
    g = torch.Generator().manual_seed(40 + Np)
    qkv = torch.randn(B, Np, 3 * H * 64, generator=g).to(BF).to(DEV)
    sin, cos = (t.to(DEV) for t in K.rope_tables(Nc))
    k_cache = torch.full((B, H, Nc, 64), NAN, dtype=BF, device=DEV)
    v_cache = torch.full((B, H, Nc, 64), NAN, dtype=BF, device=DEV)
    before = bits(k_cache)

    rot = dispatch.ext_prefill().prefill_rope_kv(qkv, sin, cos, k_cache,
                                                 v_cache, P)
    want = dispatch.ext().rope_qkv(qkv, sin, cos)
    assert torch.equal(bits(rot), bits(want))
    heads = rot.view(B, Np, 3, H, 64)
    for name, cache, which in (("k", k_cache, 1), ("v", v_cache, 2)):
        rows = heads[:, :P, which].transpose(1, 2)       # (B, H, P, 64)
        assert torch.equal(bits(cache[:, :, :P]), bits(rows)), name
        assert torch.equal(bits(cache[:, :, P:]), before[:, :, P:]), name


# ---------------------------------------------------------------------------
# prefill_gate_ln
# ---------------------------------------------------------------------------

# d2 = 3072 is the flagship's width and the first to take the kernel's
# re-reading path (more than 256 vectors a row)
@pytest.mark.parametrize("d2", [64, 1536, 3072])
@pytest.mark.parametrize("P", [1, 255, 256])
def test_prefill_gate_ln(d2, P):
    B, Np, Nc = 2, 256, 512
    g = torch.Generator().manual_seed(50 + d2)
    x = torch.randn(B, Np, 2 * d2, generator=g)
    x[..., :d2] = 5 * x[..., :d2] + 3        # the half that must not be read
    x = x.to(BF)
    w = (1 + 0.25 * torch.randn(d2, generator=g)).to(BF)
    hist = torch.full((B, Nc, d2), NAN, dtype=BF, device=DEV)
    before = bits(hist)

    got = dispatch.ext_prefill().prefill_gate_ln(x.to(DEV), w.to(DEV), hist,
                                                 P, 1e-5)
    assert got.shape == (B, Np, d2) and got.is_contiguous()
    want = R.layernorm_nobias(x[..., d2:].double(), w.double(), 1e-5)
    err = K.row_err(got, want)
    emu, bound = K.bounds("ln", "bf16")["y"]
    print(f"PREFILL|gate_ln|d2={d2}|P={P}|{emu:.3e}|{bound:.3e}|{err:.3e}")
    assert err <= bound
    assert torch.equal(bits(hist[:, :P]), bits(got[:, :P]))
    assert torch.equal(bits(hist[:, P:]), before[:, P:])


# ---------------------------------------------------------------------------
# the whole prefill
# ---------------------------------------------------------------------------

SEQ_LEN = 512
PS = [1, 64, 65, 255, 256, 257, 511]
BS = [1, 3]


@functools.lru_cache(maxsize=None)
def _model():
    # the model of tests/test_decode_prefill.py with the kernels' dim_head
    from progen_amd import ProGenBase, ProGenConfig
    cfg = ProGenConfig(num_tokens=256, dim=128, depth=3, dim_head=64, heads=2,
                       window_size=64, seq_len=SEQ_LEN, ff_glu=True,
                       global_mlp_depth=1, shift_tokens=True)
    torch.manual_seed(7)
    m = ProGenBase(cfg).to(device=DEV, dtype=BF).eval()
    m.rotary_sin = m.rotary_sin.float()
    m.rotary_cos = m.rotary_cos.float()
    return m


@functools.lru_cache(maxsize=None)
def _model64():
    """the same bf16-rounded weights on the CPU, in fp64"""
    m = copy.deepcopy(_model()).to(device="cpu", dtype=torch.float64)
    m.rotary_sin = m.rotary_sin.float()
    m.rotary_cos = m.rotary_cos.float()
    return m


@functools.lru_cache(maxsize=None)
def _tokens(B):
    g = torch.Generator().manual_seed(100 + B)
    return torch.randint(1, 256, (B, SEQ_LEN), generator=g)


def _tensors(cache):
    """(name, tensor, dimension its positions run along or None)"""
    out = [(f"k{i}", t, 2) for i, t in enumerate(cache.k)]
    out += [(f"v{i}", t, 2) for i, t in enumerate(cache.v)]
    out += [(f"gate_hist{i}", t, 1) for i, t in enumerate(cache.gate_hist)
            if t is not None]
    out += [(f"attn_prev{i}", t, None) for i, t in enumerate(cache.attn_prev)]
    out += [(f"ff_prev{i}", t, None) for i, t in enumerate(cache.ff_prev)]
    return out


def _snapshot(cache, P):
    """the cache's state after P positions, on the CPU"""
    return {name: (t if dim is None else t.narrow(dim, 0, P)).cpu().clone()
            for name, t, dim in _tensors(cache)}


@functools.lru_cache(maxsize=None)
def _stepped(B):
    """{P: (cache snapshot after P fused steps, logits of step P-1, logits
    of step P)} on the GPU"""
    m, tok = _model(), _tokens(B).to(DEV)
    cache = decode.DecodeCache(m, batch=B)
    pos = torch.zeros((), dtype=torch.long, device=DEV)
    snaps, logits = {}, {}
    for p in range(SEQ_LEN):
        out = decode.forward_step_fused(m, tok[:, p].contiguous(), cache, pos)
        pos += 1
        if p + 1 in PS or p in PS:
            logits[p] = out.cpu()
        if p + 1 in PS:
            snaps[p + 1] = _snapshot(cache, p + 1)
    return {P: (snaps[P], logits[P - 1], logits[P]) for P in PS}


@functools.lru_cache(maxsize=None)
def _oracle(B):
    """{P: cache snapshot after P steps of the fp64 CPU ``forward_step``}"""
    m, tok = _model64(), _tokens(B)
    cache = decode.DecodeCache(m, batch=B)
    snaps = {}
    for p in range(max(PS)):
        decode.forward_step(m, tok[:, p], cache)
        if p + 1 in PS:
            snaps[p + 1] = _snapshot(cache, p + 1)
    return snaps


def _cache_err(snap, oracle):
    """one figure for a cache: its worst tensor's rel_err"""
    return max(rel_err(snap[name], oracle[name]) for name in oracle)


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("P", PS)
def test_prefill_matches_the_fused_step_loop(P, B):
    m, tok = _model(), _tokens(B)
    step_snap, step_logits, step_next = _stepped(B)[P]
    oracle = _oracle(B)[P]

    cache = decode.DecodeCache(m, batch=B)
    pos = torch.zeros((), dtype=torch.long, device=DEV)
    logits = decode.prefill(m, tok[:, :P], cache, pos, want_logits=True)
    assert cache.pos == P == int(pos)
    snap = _snapshot(cache, P)
    nxt = decode.forward_step_fused(m, tok[:, P].to(DEV), cache, pos)

    e_logits = rel_err(logits, step_logits)
    e_next = rel_err(nxt, step_next)
    e_prefill = _cache_err(snap, oracle)
    e_steps = _cache_err(step_snap, oracle)
    print(f"PREFILL|whole|P={P}|B={B}|want_logits={e_logits:.3e}|"
          f"next_step={e_next:.3e}|cache_prefill={e_prefill:.3e}|"
          f"cache_steps={e_steps:.3e}")
    assert e_logits < 6e-2
    assert e_next < 6e-2
    assert e_prefill <= 2 * e_steps


def test_sample_cached_prefill_under_the_captured_fused_step(monkeypatch):
    """17-token prime, 40 sampled tokens on the captured fused step with the
    decode linear kernel. Token equality with the step-loop run is not
    demanded in bf16 (a near-tie may flip); the logits the first token is
    sampled from are held to the 6e-2 bound."""
    m = _model()
    torch.manual_seed(11)
    prime = torch.randint(1, 256, (17,))
    n = 40
    monkeypatch.setattr(decode, "PREFILL_MIN_TOKENS", 2)
    assert decode.prefill_supported(m, 17, DEV)

    made, first = [], []
    real_graph, real_prefill = decode.GraphedDecodeStep, decode.prefill

    def graphed(*a, **k):
        made.append(real_graph(*a, **k))
        return made[-1]

    def prefill(*a, **k):
        first.append(real_prefill(*a, **k))
        return first[-1]

    monkeypatch.setattr(decode, "GraphedDecodeStep", graphed)
    monkeypatch.setattr(decode, "prefill", prefill)
    out = decode.sample_cached(m, prime, len(prime) + n, top_k=25,
                               generator=torch.Generator().manual_seed(3),
                               graph=True, fused=True, fused_linear=True,
                               prefill=True)
    assert len(made) == 1 and len(first) == 1
    g = made[0]
    assert g.fused and g.fused_linear
    assert torch.equal(out[:17], prime)
    # every sampled token but the last is stepped on (fewer only if a second
    # pad ends the row early)
    assert int(g.pos_dev) == g.cache.pos
    assert len(prime) <= g.cache.pos <= len(prime) + n - 1

    cache = decode.DecodeCache(m, batch=1)
    pos = torch.zeros((), dtype=torch.long, device=DEV)
    for p in range(len(prime)):
        want = decode.forward_step_fused(m, prime[p:p + 1].to(DEV), cache, pos,
                                         fused_linear=True)
        pos += 1
    err = rel_err(first[0], want)
    print(f"PREFILL|first_token_logits|{err:.3e}")
    assert err < 6e-2


@pytest.mark.parametrize("device_sampling", [False, True])
def test_sample_cached_batch_prefills_the_common_prefix(monkeypatch,
                                                        device_sampling):
    """Ragged primes of 10, 13 and 30 tokens on the captured fused step: the
    9 common positions are prefilled, the step is captured there, the primes
    come back intact and the positions agree at the end."""
    m = _model()
    g = torch.Generator().manual_seed(13)
    primes = [torch.randint(1, 256, (n,), generator=g) for n in (10, 13, 30)]
    monkeypatch.setattr(decode, "PREFILL_MIN_TOKENS", 2)
    made, filled = [], []
    real_graph, real_prefill = decode.GraphedDecodeStep, decode.prefill

    def graphed(*a, **k):
        made.append((real_graph(*a, **k), k["start_pos"]))
        return made[-1][0]

    def prefill(model, tokens, *a, **k):
        filled.append(tuple(tokens.shape))
        return real_prefill(model, tokens, *a, **k)

    monkeypatch.setattr(decode, "GraphedDecodeStep", graphed)
    monkeypatch.setattr(decode, "prefill", prefill)
    out = decode.sample_cached_batch(m, primes, 48, graph=True, fused=True,
                                     fused_linear=True, prefill=True,
                                     device_sampling=device_sampling)
    assert filled == [(3, 9)]
    (gs, start), = made
    assert start == 9
    assert int(gs.pos_dev) == gs.cache.pos <= 47
    for row, p in zip(out, primes):
        assert torch.equal(row[:len(p)], p)
    assert out.shape == (3, 48)


def test_prefill_is_refused_where_the_kernels_do_not_serve():
    """fp32 parameters on a GPU: the samplers keep their step loop."""
    from progen_amd import ProGenBase
    m32 = ProGenBase(_model().cfg).to(DEV).eval()
    assert not decode.prefill_supported(m32, 64, DEV)
    assert decode.prefill_supported(_model(), decode.PREFILL_MIN_TOKENS, DEV)
    assert not decode.prefill_supported(_model(),
                                        decode.PREFILL_MIN_TOKENS - 1, DEV)
