"""GPU: the fused decode kernels (progen_amd/ops/hip/decode_*.hip) against
the fp32 reference ops run on the same dtype-rounded inputs, the whole
fused step against the HIP full forward, and its hipGraph capture.

Tolerances and ``rel_err`` are those of tests/test_gpu_kernels.py: 2e-2 for
bf16, 1e-5 for fp32, max-abs error over the reference's max-abs value.

Cache rows a step must not read (after ``pos``, before the band start, and
row ``pos`` itself, which the kernels take from registers) are NaN before
each launch: a finite result shows they were not read. No test launches a
kernel with a position outside [0, N).
"""

import pytest
import torch

from progen_amd.ops import functional as OF, reference as R

pytestmark = pytest.mark.gpu

DTYPES = [(torch.bfloat16, 2e-2), (torch.float32, 1e-5)]
NAN = float("nan")


def dev():
    return torch.device("cuda:0")


def rel_err(got, want):
    got = got.float().cpu()
    want = want.float().cpu()
    denom = want.abs().max().clamp_min(1e-6)
    return ((got - want).abs().max() / denom).item()


def bits(x):
    """Raw storage bits, so that NaN rows compare equal to themselves."""
    return x.cpu().view(torch.int16 if x.dtype == torch.bfloat16
                        else torch.int32)


def f32(x):
    return None if x is None else x.detach().float().cpu()


# ---------------------------------------------------------------------------
# dec_ln_shift
# ---------------------------------------------------------------------------

# D = 4096 takes the kernel's second path (rows wider than 2048 elements
# re-read the stream instead of keeping one chunk per thread in registers)
@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("D", [128, 1536, 4096])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shift", [True, False])
@pytest.mark.parametrize("use_res", [True, False])
def test_dec_ln_shift(dtype, tol, D, B, shift, use_res):
    torch.manual_seed(0)
    h = torch.randn(B, D, device=dev()).to(dtype)
    res = torch.randn(B, D, device=dev()).to(dtype) if use_res else None
    g = torch.randn(D, device=dev()).to(dtype)
    prev = torch.randn(B, D, device=dev()).to(dtype)
    h32, res32, g32, prev32 = f32(h), f32(res), f32(g), f32(prev)

    y = OF.decode_ln_shift(h, res, g, prev, shift=shift)
    y32 = R.decode_ln_shift(h32, res32, g32, prev32, shift)

    assert y.dtype == dtype and y.shape == (B, D)
    assert rel_err(y, y32) < tol
    assert rel_err(h, h32) < tol
    assert rel_err(prev, prev32) < tol
    if shift:
        # the shifted half is a copy of the previous row, bit for bit
        assert torch.equal(y[:, :D // 2].float().cpu(), y32[:, :D // 2])


@pytest.mark.parametrize("dtype,tol", DTYPES)
def test_dec_ln_shift_without_prev(dtype, tol):
    """The final norm: no shift, no previous row to update."""
    torch.manual_seed(1)
    h = torch.randn(3, 128, device=dev()).to(dtype)
    res = torch.randn(3, 128, device=dev()).to(dtype)
    g = torch.randn(128, device=dev()).to(dtype)
    h32, res32, g32 = f32(h), f32(res), f32(g)
    y = OF.decode_ln_shift(h, res, g, None, shift=False)
    y32 = R.decode_ln_shift(h32, res32, g32, None, False)
    assert rel_err(y, y32) < tol
    assert rel_err(h, h32) < tol


# ---------------------------------------------------------------------------
# dec_attn
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("window,N,positions", [
    (64, 256, [0, 63, 64, 127, 128, 255]),
    (256, 512, [0, 255, 256, 511]),
])
def test_dec_attn(dtype, tol, window, N, positions):
    torch.manual_seed(2)
    B, H = 2, 2
    sin, cos = R.fixed_pos_embedding(N, 64)
    sin_d, cos_d = sin.to(dev()), cos.to(dev())
    k0 = torch.randn(B, H, N, 64).to(dtype)
    v0 = torch.randn(B, H, N, 64).to(dtype)
    for p in positions:
        qkv = torch.randn(B, 3 * H * 64).to(dtype)
        start = max(0, (p // window) * window - window)
        k_in, v_in = k0.clone(), v0.clone()
        for c in (k_in, v_in):
            c[:, :, p:] = NAN       # rows > pos, and row pos itself
            c[:, :, :start] = NAN   # rows before the band
        k_ref, v_ref = k_in.float(), v_in.float()
        want = R.decode_attention(qkv.float(), sin, cos, torch.tensor(p),
                                  k_ref, v_ref, window)

        k_d, v_d = k_in.to(dev()), v_in.to(dev())
        pos = torch.tensor(p, dtype=torch.long, device=dev())
        got = OF.decode_attention(qkv.to(dev()), sin_d, cos_d, pos, k_d, v_d,
                                  window)
        assert got.shape == (B, H * 64) and got.dtype == dtype
        assert torch.isfinite(got).all(), p
        assert rel_err(got, want) < tol, p
        for after, before, ref in ((k_d, k_in, k_ref), (v_d, v_in, v_ref)):
            others = [i for i in range(N) if i != p]
            assert torch.equal(bits(after)[:, :, others],
                               bits(before)[:, :, others]), p
            assert rel_err(after[:, :, p], ref[:, :, p]) < tol, p
        assert int(pos) == p


# ---------------------------------------------------------------------------
# dec_sgu
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("d2", [64, 320])
def test_dec_sgu(dtype, tol, d2):
    torch.manual_seed(3)
    B, N = 2, 256
    g = torch.randn(d2).to(dtype)
    w = (torch.randn(N, N) / 16).to(dtype)
    bias = torch.randn(N, 1).to(dtype)
    hist0 = torch.randn(B, N, d2).to(dtype)
    for p in (0, 1, 255):
        h = torch.randn(B, 2 * d2).to(dtype)
        hist_in = hist0.clone()
        hist_in[:, p:] = NAN        # rows > pos, and row pos itself
        hist_ref = hist_in.float()
        want = R.decode_sgu(h.float(), g.float(), hist_ref, w.float(),
                            bias.float(), torch.tensor(p))

        hist_d = hist_in.to(dev())
        pos = torch.tensor(p, dtype=torch.long, device=dev())
        got = OF.decode_sgu(h.to(dev()), g.to(dev()), hist_d, w.to(dev()),
                            bias.to(dev()), pos)
        assert got.shape == (B, d2) and got.dtype == dtype
        assert torch.isfinite(got).all(), p
        assert rel_err(got, want) < tol, p
        others = [i for i in range(N) if i != p]
        assert torch.equal(bits(hist_d)[:, others], bits(hist_in)[:, others]), p
        assert rel_err(hist_d[:, p], hist_ref[:, p]) < tol, p


# ---------------------------------------------------------------------------
# the whole fused step
# ---------------------------------------------------------------------------

def test_fused_decode_matches_hip_forward():
    """The model and bound of
    test_gpu_kernels.py::test_cached_decode_matches_hip_forward."""
    from progen_amd import ProGenBase, ProGenConfig
    from progen_amd.decode import DecodeCache, forward_step_fused
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
        rows.append(forward_step_fused(m, seq[p:p + 1], cache, pos))
        pos += 1
    inc = torch.cat(rows, dim=0).float()
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


def _prefill_fused(m, prime):
    from progen_amd.decode import DecodeCache, forward_step_fused
    cache = DecodeCache(m, batch=1)
    pos = torch.zeros((), dtype=torch.long, device="cuda")
    logits = None
    for p in range(len(prime)):
        logits = forward_step_fused(m, prime[p:p + 1].cuda(), cache, pos)
        pos += 1
    return cache, pos, logits.cpu().float().argmax(dim=-1)


def test_graphed_fused_decode_matches_uncaptured():
    """The kernels use no atomics, so a replay reproduces the uncaptured
    step bit for bit: greedy tokens are equal, not merely close."""
    from progen_amd.decode import GraphedDecodeStep, forward_step_fused
    m = _graph_model()
    torch.manual_seed(11)
    prime = torch.randint(1, 256, (17,))
    n = 40

    cache, pos, tok = _prefill_fused(m, prime)
    want = []
    for _ in range(n):
        want.append(int(tok))
        logits = forward_step_fused(m, tok.cuda(), cache, pos)
        pos += 1
        tok = logits.cpu().float().argmax(dim=-1)

    cache, pos, tok = _prefill_fused(m, prime)
    g = GraphedDecodeStep(m, cache, start_pos=len(prime), fused=True)
    got = []
    for _ in range(n):
        got.append(int(tok))
        tok = g.step(tok).cpu().float().argmax(dim=-1)
    assert got == want, (got, want)
    assert int(g.pos_dev) == len(prime) + n == cache.pos


def test_graphed_step_refuses_to_run_past_seq_len():
    """The host-side count stops the replay that would run at seq_len; the
    device position shows that nothing was replayed."""
    from progen_amd.decode import DecodeCache, GraphedDecodeStep
    m = _graph_model()
    last = m.cfg.seq_len - 1
    cache = DecodeCache(m, batch=1)
    g = GraphedDecodeStep(m, cache, start_pos=last, fused=True)
    assert int(g.pos_dev) == last
    tok = torch.tensor([7])
    logits = g.step(tok).cpu()
    assert torch.isfinite(logits).all()
    assert int(g.pos_dev) == m.cfg.seq_len
    with pytest.raises(IndexError):
        g.step(tok)
    assert int(g.pos_dev) == m.cfg.seq_len
    assert torch.equal(g.static_logits.cpu(), logits)
