"""GPU numerics tests: every HIP kernel vs the plain PyTorch fp32
reference (ops/reference.py) on the same (bf16-rounded) inputs.

All tests are @pytest.mark.gpu — run on an MI355X via gpurun; skipped on
the CPU-only container (tests/conftest.py).
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from progen_amd.ops import dispatch, functional as OF, reference as R


def dev():
    return torch.device("cuda:0")


def rel_err(got, want):
    got = got.float().cpu()
    want = want.float().cpu()
    denom = want.abs().max().clamp_min(1e-6)
    return ((got - want).abs().max() / denom).item()


# ---------------------------------------------------------------------------
# ln_shift
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,tol", [(torch.bfloat16, 2e-2), (torch.float32, 1e-5)])
@pytest.mark.parametrize("shift", [True, False])
def test_ln_shift_fwd_bwd(dtype, tol, shift):
    torch.manual_seed(0)
    B, N, D = 2, 32, 128
    x = torch.randn(B, N, D, device=dev(), dtype=dtype, requires_grad=True)
    g = torch.randn(D, device=dev(), dtype=dtype, requires_grad=True)

    y = OF.ln_shift(x, g, shift=shift)
    dy = torch.randn_like(y)
    y.backward(dy)

    x32 = x.detach().float().cpu().requires_grad_(True)
    g32 = g.detach().float().cpu().requires_grad_(True)
    y32 = R.ln_shift(x32, g32, shift=shift)
    y32.backward(dy.float().cpu())

    assert rel_err(y, y32) < tol
    assert rel_err(x.grad, x32.grad) < tol * 3
    assert rel_err(g.grad, g32.grad) < tol * 3


@pytest.mark.parametrize("dtype,tol", [(torch.bfloat16, 2e-2), (torch.float32, 1e-5)])
@pytest.mark.parametrize("shift", [True, False])
@pytest.mark.parametrize("use_ds", [True, False])
def test_ln_shift_res_fwd_bwd(dtype, tol, shift, use_ds):
    torch.manual_seed(2)
    B, N, D = 2, 32, 128
    x = torch.randn(B, N, D, device=dev(), dtype=dtype, requires_grad=True)
    r = torch.randn(B, N, D, device=dev(), dtype=dtype, requires_grad=True)
    g = torch.randn(D, device=dev(), dtype=dtype, requires_grad=True)

    y, s = OF.ln_shift_res(x, r, g, shift=shift)
    dy = torch.randn_like(y)
    if use_ds:
        ds = torch.randn_like(s)
        torch.autograd.backward([y, s], [dy, ds])
    else:
        y.backward(dy)

    x32 = x.detach().float().cpu().requires_grad_(True)
    r32 = r.detach().float().cpu().requires_grad_(True)
    g32 = g.detach().float().cpu().requires_grad_(True)
    s32 = x32 + r32
    y32 = R.ln_shift(s32, g32, shift=shift)
    if use_ds:
        torch.autograd.backward([y32, s32], [dy.float().cpu(), ds.float().cpu()])
    else:
        y32.backward(dy.float().cpu())

    assert rel_err(y, y32) < tol
    assert rel_err(s, s32) < tol
    assert rel_err(x.grad, x32.grad) < tol * 3
    assert rel_err(r.grad, r32.grad) < tol * 3
    assert rel_err(g.grad, g32.grad) < tol * 3


# ---------------------------------------------------------------------------
# glu / gelu
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,tol", [(torch.bfloat16, 2e-2), (torch.float32, 1e-5)])
def test_glu_fwd_bwd(dtype, tol):
    torch.manual_seed(1)
    h = torch.randn(2, 16, 256, device=dev(), dtype=dtype, requires_grad=True)
    y = OF.glu_gelu(h)
    dy = torch.randn_like(y)
    y.backward(dy)

    h32 = h.detach().float().cpu().requires_grad_(True)
    y32 = R.glu_gelu(h32)
    y32.backward(dy.float().cpu())
    assert rel_err(y, y32) < tol
    assert rel_err(h.grad, h32.grad) < tol * 3


@pytest.mark.parametrize("dtype,tol", [(torch.bfloat16, 2e-2), (torch.float32, 1e-5)])
def test_gelu_fwd_bwd(dtype, tol):
    torch.manual_seed(2)
    h = torch.randn(2, 16, 128, device=dev(), dtype=dtype, requires_grad=True)
    y = OF.gelu(h)
    dy = torch.randn_like(y)
    y.backward(dy)
    h32 = h.detach().float().cpu().requires_grad_(True)
    y32 = R.gelu(h32)
    y32.backward(dy.float().cpu())
    assert rel_err(y, y32) < tol
    assert rel_err(h.grad, h32.grad) < tol * 3


# ---------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,tol", [(torch.bfloat16, 1e-2), (torch.float32, 1e-5)])
def test_cross_entropy_fwd_bwd(dtype, tol):
    torch.manual_seed(3)
    B, N, V = 3, 33, 256
    logits = torch.randn(B, N, V, device=dev(), dtype=dtype,
                         requires_grad=True) * 3
    logits.retain_grad()
    targets = torch.randint(0, V, (B, N), device=dev())
    targets[:, -5:] = 0  # pad tail -> EOS mask path

    loss = OF.cross_entropy(logits, targets)
    loss.backward()

    l32 = logits.detach().float().cpu().requires_grad_(True)
    loss32 = R.cross_entropy(l32, targets.cpu())
    loss32.backward()
    assert abs(loss.item() - loss32.item()) < tol * 5
    assert rel_err(logits.grad, l32.grad) < tol * 5


# ---------------------------------------------------------------------------
# local attention
# ---------------------------------------------------------------------------

ATTN_CASES = [
    # (B, N, heads, wsz)
    (2, 128, 2, 64),     # 2 windows, tiny
    (1, 256, 3, 64),     # window 0 quirk + several windows
    (2, 1024, 8, 256),   # ProGen-small shape
    (1, 1024, 4, 512),   # default.toml window (wsz > 256 -> chunk rounds)
]


@pytest.mark.parametrize("B,N,H,wsz", ATTN_CASES)
def test_attn_fwd(B, N, H, wsz):
    torch.manual_seed(4)
    qkv = (torch.randn(B, N, 3 * H * 64, device=dev()) / 8.0).to(torch.bfloat16)
    sin, cos = R.fixed_pos_embedding(N, 64, device=dev())
    out = OF.local_attention(qkv, sin, cos, H, wsz)

    want = R.local_attention(qkv.float().cpu(), sin.cpu(), cos.cpu(), H, wsz)
    assert rel_err(out, want) < 2e-2


@pytest.mark.parametrize("B,N,H,wsz", ATTN_CASES)
def test_attn_bwd(B, N, H, wsz):
    torch.manual_seed(5)
    qkv = ((torch.randn(B, N, 3 * H * 64, device=dev()) / 8.0)
           .to(torch.bfloat16).requires_grad_(True))
    sin, cos = R.fixed_pos_embedding(N, 64, device=dev())
    out = OF.local_attention(qkv, sin, cos, H, wsz)
    dout = (torch.randn_like(out) / 8.0).to(torch.bfloat16)
    out.backward(dout)

    q32 = qkv.detach().float().cpu().requires_grad_(True)
    want = R.local_attention(q32, sin.cpu(), cos.cpu(), H, wsz)
    want.backward(dout.float().cpu())
    assert rel_err(qkv.grad, q32.grad) < 3e-2


def test_attn_window0_zero_lookback_quirk_gpu():
    """The kernel must reproduce the unmasked zero-key softmax dilution
    in window 0 (progen.py:90-96)."""
    torch.manual_seed(6)
    B, N, H, wsz = 1, 64, 1, 64
    qkv = (torch.randn(B, N, 3 * H * 64, device=dev()) / 8.0).to(torch.bfloat16)
    sin, cos = R.fixed_pos_embedding(N, 64, device=dev())
    out = OF.local_attention(qkv, sin, cos, H, wsz)
    want = R.local_attention(qkv.float().cpu(), sin.cpu(), cos.cpu(), H, wsz)
    # row 0 is maximally diluted by the 64 zero keys -- the sharpest test
    assert rel_err(out[:, 0], want[:, 0]) < 2e-2


# ---------------------------------------------------------------------------
# fused adamw
# ---------------------------------------------------------------------------

def test_fused_adamw_matches_eager():
    import copy

    from progen_amd import ProGenBase, ProGenConfig
    from progen_amd.optim import ProGenAdamW
    from progen_amd.utils import compute_loss

    cfg = ProGenConfig(num_tokens=64, dim=64, seq_len=64, depth=2,
                       window_size=64, global_mlp_depth=1, heads=1, dim_head=64)
    torch.manual_seed(7)
    m_gpu = ProGenBase(cfg).to(device=dev(), dtype=torch.bfloat16)
    m_gpu.rotary_sin = m_gpu.rotary_sin.float()
    m_gpu.rotary_cos = m_gpu.rotary_cos.float()
    m_cpu = copy.deepcopy(m_gpu).float().cpu()

    o_gpu = ProGenAdamW(m_gpu, lr=1e-3, max_grad_norm=0.5)
    o_cpu = ProGenAdamW(m_cpu, lr=1e-3, max_grad_norm=0.5)
    # identical synthetic gradient on both
    torch.manual_seed(8)
    fake = torch.randn(o_cpu.space.flat_grad.shape)
    o_gpu.space.flat_grad.copy_(fake.to(dev()).to(o_gpu.space.flat_grad.dtype))
    o_cpu.space.flat_grad.copy_(fake)
    # account for bf16 grad rounding in the oracle
    o_cpu.space.flat_grad.copy_(
        o_gpu.space.flat_grad.float().cpu())

    o_gpu.step()
    o_cpu.step()
    err = (o_gpu.master.float().cpu() - o_cpu.master).abs().max().item()
    assert err < 1e-5

    # also end-to-end micro step runs
    data = torch.randint(1, 64, (2, 65), device=dev())
    data[:, 0] = 0
    compute_loss(m_gpu, data).backward()
    o_gpu.micro_step()
    torch.cuda.synchronize()


def test_fused_adamw_shard_off_matches_full():
    """ZeRO-1 kernel path (parallel/zero1.py::_step_hip): updating the
    flat space as two half-shards with shard-clipped chunk tables and
    shard_off must reproduce the full-space fused update bitwise
    (single-GPU stand-in for the world=2 sharding, which RCCL cannot
    run on one device)."""
    import copy

    from progen_amd import ProGenBase, ProGenConfig
    from progen_amd.ops import dispatch
    from progen_amd.optim import ProGenAdamW

    cfg = ProGenConfig(num_tokens=64, dim=64, seq_len=64, depth=2,
                       window_size=64, global_mlp_depth=1, heads=1, dim_head=64)
    torch.manual_seed(17)
    m_a = ProGenBase(cfg).to(device=dev(), dtype=torch.bfloat16)
    m_a.rotary_sin = m_a.rotary_sin.float()
    m_a.rotary_cos = m_a.rotary_cos.float()
    m_b = copy.deepcopy(m_a)

    # no grad clipping: the grad-norm reduce is atomicAdd-ordered and
    # its last-ulp nondeterminism would break the bitwise comparison
    # (clip correctness is covered by test_fused_adamw_matches_eager)
    o_full = ProGenAdamW(m_a, lr=1e-3, max_grad_norm=None)
    o_shard = ProGenAdamW(m_b, lr=1e-3, max_grad_norm=None)
    torch.manual_seed(18)
    fake = torch.randn(o_full.space.flat_grad.shape, device=dev())
    o_full.space.flat_grad.copy_(fake.to(o_full.space.flat_grad.dtype))
    o_shard.space.flat_grad.copy_(o_full.space.flat_grad)

    o_full.step()

    # shard o_shard's update into two halves by hand
    C = dispatch.ext()
    n = o_shard.space.numel
    lo_hi = [(0, n // 2), (n // 2, n)]
    clip = torch.ones(1, device=dev())
    o_shard.step_count += 1
    for i, (lo, hi) in enumerate(lo_hi):
        starts = o_shard.chunk_starts.clamp(min=lo, max=hi)
        ends = o_shard.chunk_ends.clamp(min=lo, max=hi)
        keep = ends > starts
        # each shard call must increment step_dev exactly once overall:
        # emulate by resetting after the first call
        step_before = o_shard.step_dev.clone()
        C.fused_adamw(
            o_shard.master[lo:hi], o_shard.space.flat,
            o_shard.space.flat_grad,
            o_shard.exp_avg[lo:hi], o_shard.exp_avg_sq[lo:hi],
            starts[keep].clone(), ends[keep].clone(),
            o_shard.chunk_decay[keep].clone(),
            1e-3, 0.9, 0.999, 1e-8, 1e-3, o_shard.step_dev,
            1.0, clip, shard_off=lo)
        if i == 0:
            o_shard.step_dev.copy_(step_before)  # undo duplicate inc
    torch.cuda.synchronize()

    assert torch.equal(o_full.master, o_shard.master)
    assert torch.equal(o_full.exp_avg, o_shard.exp_avg)
    assert torch.equal(o_full.space.flat, o_shard.space.flat)


# ---------------------------------------------------------------------------
# full model parity GPU(bf16 kernels) vs CPU(fp32 reference)
# ---------------------------------------------------------------------------

def test_model_forward_parity():
    import copy

    from progen_amd import ProGenBase, ProGenConfig
    cfg = ProGenConfig(num_tokens=256, dim=128, seq_len=256, depth=3,
                       window_size=64, global_mlp_depth=1, heads=2, dim_head=64)
    torch.manual_seed(9)
    m = ProGenBase(cfg)
    m_cpu = copy.deepcopy(m)
    m_gpu = m.to(device=dev(), dtype=torch.bfloat16)
    m_gpu.rotary_sin = m_gpu.rotary_sin.float()
    m_gpu.rotary_cos = m_gpu.rotary_cos.float()

    x = torch.randint(1, 256, (2, 256))
    out_gpu = m_gpu(x.to(dev())).float().cpu()
    out_cpu = m_cpu(x)
    assert rel_err(out_gpu, out_cpu) < 6e-2  # bf16 across 3 layers


def test_training_loss_decreases():
    from progen_amd import ProGenBase, ProGenConfig
    from progen_amd.optim import ProGenAdamW
    from progen_amd.utils import compute_loss

    cfg = ProGenConfig(num_tokens=256, dim=128, seq_len=256, depth=2,
                       window_size=64, global_mlp_depth=1, heads=2, dim_head=64)
    torch.manual_seed(10)
    m = ProGenBase(cfg).to(device=dev(), dtype=torch.bfloat16)
    m.rotary_sin = m.rotary_sin.float()
    m.rotary_cos = m.rotary_cos.float()
    opt = ProGenAdamW(m, lr=3e-4, max_grad_norm=0.5)
    data = torch.randint(1, 256, (4, 257), device=dev())
    data[:, 0] = 0
    losses = []
    for _ in range(30):
        loss = compute_loss(m, data)
        loss.backward()
        opt.micro_step()
        losses.append(loss.item())
    assert losses[-1] < losses[0] * 0.7, losses[::10]


# ---------------------------------------------------------------------------
# SGU spatial gating kernels
# ---------------------------------------------------------------------------

def test_sgu_kernels_fwd_bwd():
    torch.manual_seed(11)
    B, N, H = 2, 256, 256  # H = full hidden (split into xa/gate halves)
    x = (torch.randn(B, N, H, device=dev()) / 4.0).to(torch.bfloat16)
    x.requires_grad_(True)
    g = torch.randn(H // 2, device=dev(), dtype=torch.bfloat16)
    g.requires_grad_(True)
    W = (torch.randn(N, N, device=dev()) * 1e-3).to(torch.bfloat16)
    W.requires_grad_(True)
    b = torch.ones(N, 1, device=dev(), dtype=torch.bfloat16)
    b.requires_grad_(True)

    out = OF.sgu_gate(x, g, W, b)
    dy = (torch.randn_like(out) / 4.0).to(torch.bfloat16)
    out.backward(dy)

    x32 = x.detach().float().cpu().requires_grad_(True)
    g32 = g.detach().float().cpu().requires_grad_(True)
    W32 = W.detach().float().cpu().requires_grad_(True)
    b32 = b.detach().float().cpu().requires_grad_(True)
    out32 = R.sgu_gate(x32, g32, W32, b32)
    out32.backward(dy.float().cpu())

    assert rel_err(out, out32) < 2e-2
    assert rel_err(x.grad, x32.grad) < 3e-2
    assert rel_err(g.grad, g32.grad) < 3e-2
    assert rel_err(W.grad, W32.grad) < 3e-2
    assert rel_err(b.grad, b32.grad) < 3e-2


def test_sgu_causality_gpu():
    torch.manual_seed(12)
    B, N, H = 1, 256, 128
    x = (torch.randn(B, N, H, device=dev()) / 4.0).to(torch.bfloat16)
    g = torch.ones(H // 2, device=dev(), dtype=torch.bfloat16)
    W = (torch.randn(N, N, device=dev()) * 1e-2).to(torch.bfloat16)
    b = torch.ones(N, 1, device=dev(), dtype=torch.bfloat16)
    base = OF.sgu_gate(x, g, W, b)
    x2 = x.clone()
    p = 100
    x2[0, p] += 1.0
    out2 = OF.sgu_gate(x2, g, W, b)
    d = (base[0, :p].float() - out2[0, :p].float()).abs().max().item()
    assert d == 0.0, d


# ---------------------------------------------------------------------------
# hipGraph-captured step == eager step (training parity)
# ---------------------------------------------------------------------------

def test_graphed_step_matches_eager():
    """The captured graph must reproduce eager training exactly: same
    data stream from the same init -> same parameters after 5 steps."""
    import copy

    from progen_amd import ProGenBase, ProGenConfig
    from progen_amd.optim import ProGenAdamW
    from progen_amd.runtime import GraphedTrainStep
    from progen_amd.utils import compute_loss

    cfg = ProGenConfig(num_tokens=256, dim=128, seq_len=256, depth=2,
                       window_size=64, global_mlp_depth=1, heads=2, dim_head=64)
    torch.manual_seed(21)
    m1 = ProGenBase(cfg).to(device=dev(), dtype=torch.bfloat16)
    m2 = copy.deepcopy(m1)
    o1 = ProGenAdamW(m1, lr=3e-4, max_grad_norm=0.5)
    o2 = ProGenAdamW(m2, lr=3e-4, max_grad_norm=0.5)

    torch.manual_seed(22)
    batches = [torch.randint(1, 256, (4, 257), device=dev()) for _ in range(5)]
    for b in batches:
        b[:, 0] = 0

    g = GraphedTrainStep(m1, o1, None, 4, 256, dev())
    losses_g = []
    for b in batches:
        losses_g.append(g.run(b).item())

    losses_e = []
    for b in batches:
        o2.zero_grad()
        loss = compute_loss(m2, b)
        loss.backward()
        o2.step()
        losses_e.append(loss.item())

    np.testing.assert_allclose(losses_g, losses_e, rtol=5e-2)
    # bf16 backward is not bitwise deterministic across runs (hipBLASLt
    # split-K); after 5 steps allow update-scale drift
    err = (o1.master - o2.master).abs().max().item()
    assert err < 2e-3, err
    # device step counters advanced identically
    assert int(o1.step_dev.item()) == 5


def test_default_toml_config_train_step():
    """The reference default.toml config (window_size=512 > the 256-row
    block: chunk-round path) must train end-to-end on the kernels."""
    from progen_amd import ProGenBase, ProGenConfig
    from progen_amd.optim import ProGenAdamW
    from progen_amd.utils import compute_loss

    cfg = ProGenConfig(num_tokens=256, dim=512, depth=6, heads=8, dim_head=64,
                       window_size=512, seq_len=1024)
    torch.manual_seed(31)
    m = ProGenBase(cfg).to(device=dev(), dtype=torch.bfloat16)
    opt = ProGenAdamW(m, lr=3e-4, max_grad_norm=0.5)
    data = torch.randint(1, 256, (4, 1025), device=dev())
    data[:, 0] = 0
    losses = []
    for _ in range(8):
        loss = compute_loss(m, data)
        loss.backward()
        opt.micro_step()
        losses.append(loss.item())
    assert all(np.isfinite(losses))
    assert losses[-1] < losses[0]


# ---------------------------------------------------------------------------
# cached incremental decode on GPU (torch ops) vs the HIP full forward
# ---------------------------------------------------------------------------

def test_cached_decode_matches_hip_forward():
    from progen_amd import ProGenBase, ProGenConfig
    from progen_amd.decode import DecodeCache, forward_step
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
    rows = [forward_step(m, seq[p:p + 1], cache) for p in range(256)]
    inc = torch.cat(rows, dim=0).float()
    # bf16 GEMV vs HIP MFMA paths across 3 layers
    assert rel_err(inc, full) < 6e-2


def test_colsum_matches_torch():
    """Bias-grad column sum (ops/hip/colsum.hip) vs fp32 torch."""
    torch.manual_seed(23)
    for R, C in [(65536, 1536), (4096, 12288), (1000, 8), (64, 256)]:
        dy = (torch.randn(R, C, device=dev()) * 0.3).to(torch.bfloat16)
        got = dispatch.ext().colsum(dy)
        want = dy.float().sum(dim=0)
        assert rel_err(got, want) < 1e-3, (R, C)


def test_fused_adamw_nonfinite_skip():
    """Kernel-side step_ok guard (ops/hip/adamw.hip): an inf/NaN grad
    buffer must skip the whole update — params, master, moments and the
    DEVICE step counter all unchanged — then a healthy step applies.
    Mitigation for the open graphed-replay corruption issue
    (profiles/r02_graphed_nan_investigation.md)."""
    from progen_amd import ProGenBase, ProGenConfig
    from progen_amd.optim import ProGenAdamW

    cfg = ProGenConfig(num_tokens=64, dim=64, seq_len=64, depth=2,
                       window_size=64, global_mlp_depth=1, heads=1, dim_head=64)
    torch.manual_seed(9)
    m = ProGenBase(cfg).to(device=dev(), dtype=torch.bfloat16)
    o = ProGenAdamW(m, lr=1e-3, max_grad_norm=0.5)

    torch.manual_seed(10)
    fake = torch.randn(o.space.flat_grad.shape, device=dev())
    for bad in (float("inf"), float("nan")):
        o.space.flat_grad.copy_(fake.to(o.space.flat_grad.dtype))
        o.space.flat_grad[3] = bad
        master0 = o.master.clone()
        flat0 = o.space.flat.clone()
        v0 = o.exp_avg_sq.clone()
        step0 = int(o.step_dev.item())
        o.step()
        torch.cuda.synchronize()
        assert int(o.step_dev.item()) == step0, bad
        assert torch.equal(o.master, master0), bad
        assert torch.equal(o.space.flat, flat0), bad
        assert torch.equal(o.exp_avg_sq, v0), bad

    # healthy step still applies and advances the device counter
    o.space.flat_grad.copy_(fake.to(o.space.flat_grad.dtype))
    master0 = o.master.clone()
    o.step()
    torch.cuda.synchronize()
    assert int(o.step_dev.item()) == 1
    assert not torch.equal(o.master, master0)
    assert torch.isfinite(o.master).all()


# ---------------------------------------------------------------------------
# device guard: tensors on a device other than the current one
# ---------------------------------------------------------------------------

def test_ops_follow_their_tensors_device():
    """Each entry point launches on its tensors' device and stream, not on
    the current device's: cuda:1 inputs while cuda:0 is current."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs: runs kernels on cuda:1 with cuda:0 current")
    d1 = torch.device("cuda:1")
    torch.cuda.set_device(0)
    torch.manual_seed(31)
    x = torch.randn(1, 64, 128, device=d1, dtype=torch.bfloat16,
                    requires_grad=True)
    g = torch.randn(128, device=d1, dtype=torch.bfloat16, requires_grad=True)
    h = torch.randn(1, 64, 256, device=d1, dtype=torch.bfloat16,
                    requires_grad=True)

    y = OF.ln_shift(x, g, shift=True)
    z = OF.glu_gelu(h)
    dy, dz = torch.randn_like(y), torch.randn_like(z)
    torch.autograd.backward([y, z], [dy, dz])
    torch.cuda.synchronize(d1)
    assert torch.cuda.current_device() == 0
    assert y.device == d1 and z.device == d1

    x32 = x.detach().float().cpu().requires_grad_(True)
    g32 = g.detach().float().cpu().requires_grad_(True)
    h32 = h.detach().float().cpu().requires_grad_(True)
    y32 = R.ln_shift(x32, g32, shift=True)
    z32 = R.glu_gelu(h32)
    torch.autograd.backward([y32, z32], [dy.float().cpu(), dz.float().cpu()])

    tol = 2e-2  # the bf16 tolerance of the single-device tests above
    assert rel_err(y, y32) < tol
    assert rel_err(z, z32) < tol
    assert rel_err(x.grad, x32.grad) < tol * 3
    assert rel_err(g.grad, g32.grad) < tol * 3
    assert rel_err(h.grad, h32.grad) < tol * 3
