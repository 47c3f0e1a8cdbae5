"""GPU: every training kernel at its branch points against an fp64 oracle.

The entry points of progen_amd._C are called directly, at the smallest
shapes that reach each path of the .hip sources (slow paths, grid-stride
loops, ragged tails, partly filled attention rounds, the second dW chunk),
and each output is held, row by row, to the bound of
tests/kernel_oracle.py: twice what an emulation of the kernel's bf16
storage costs against the oracle (tests/KERNEL_TOLERANCES.md). Values
that must be exactly zero, and rows that must not change at all, are
asserted exactly. tests/test_kernel_oracle.py shows on the CPU that these
bounds reject a subtly wrong kernel. Every figure is printed as a
``KTOL|family|output|dtype|emulation|bound|measured|case`` line.
"""

import pytest
import torch

import kernel_oracle as K
from progen_amd.ops import dispatch, functional as OF, reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = ["bf16", "fp32"]
EPS = 1e-5


def C():
    return dispatch.ext()


def cu(t):
    return None if t is None else t.to(DEV)


def expect(family, dn, errs, label):
    missed = K.check(family, dn, errs, label)
    assert not missed, (family, dn, label, missed)


# ---------------------------------------------------------------------------
# ln_shift / ln_shift_res
# ---------------------------------------------------------------------------

def run_ln(case):
    inp = K.ln_inputs(case)
    x, res, g, dy, ds = (cu(inp[k]) for k in ("x", "res", "g", "dy", "ds"))
    shift = inp["shift"]
    if res is None:
        y, mean, rstd = C().ln_shift_fwd(x, g, shift, EPS)
        s = x
        dx, dw = C().ln_shift_bwd(dy, x, g, mean, rstd, shift)
    else:
        y, s, mean, rstd = C().ln_shift_res_fwd(x, res, g, shift, EPS)
        dx, dw = C().ln_shift_res_bwd(dy, ds, s, g, mean, rstd, shift)
    return dict(y=y, s=s, mean=mean, rstd=rstd, dx=dx, dw=dw)


def check_ln(case):
    got = run_ln(case)
    if case[4]:   # shift: the first row's shifted half is the zero pad
        half = case[3] // 2
        assert (got["y"][:, 0, :half] == 0).all(), case
    expect(K.ln_family(case), case[0],
           K.ln_errors(got, K.ln_oracle_of(case), case), case[1:])


@pytest.mark.parametrize("dn", DTYPES)
@pytest.mark.parametrize("width", range(5), ids=["D16", "D48", "D128",
                                                 "last_fast", "first_slow"])
def test_ln_shift_widths(dn, width):
    """D = 16, 48, 128, the last fast-path width and the first ragged
    slow-path one (Dv > 256), at (B, N) = (2, 32), (5, 1), (3, 2)."""
    shapes = K.ln_shapes(K._dt(dn))[3 * width:3 * width + 3]
    assert len({d for _, _, d in shapes}) == 1
    for shape in shapes:
        for variant in K.LN_VARIANTS:
            check_ln((dn, *shape, *variant, 0.0))


@pytest.mark.parametrize("dn", DTYPES)
def test_ln_shift_bwd_row_stride(dn):
    """R = 3 * 345 = 1035 rows on 1024 blocks: the backward's stride loop
    runs, blocks 0..10 sum dweight over two rows, and row 1034 (the last
    of its sequence) and row 1024 sit across batch boundaries of the rows
    visited first."""
    shape = K.ln_shapes(K._dt(dn))[-1]
    assert shape == (3, 345, 32)
    for variant in K.LN_VARIANTS:
        check_ln((dn, *shape, *variant, 0.0))


@pytest.mark.parametrize("dn", DTYPES)
def test_ln_shift_offset_rows(dn):
    """rows with mean 10 and std 1: var = E[x^2] - mean^2 in fp32 loses
    what the centred form keeps"""
    for case in K.ln_cases(K._dt(dn))[-2:]:
        assert case[-1] == 10.0
        check_ln(case)


@pytest.mark.parametrize("dn", DTYPES)
def test_ln_shift_autograd_wiring(dn):
    """functional.ln_shift_res hands both addends the kernel's dx and the
    weight its dw"""
    case = (dn, 3, 2, 48, True, True, True, 0.0)
    inp = K.ln_inputs(case)
    x, res, g = (cu(inp[k]).requires_grad_(True) for k in ("x", "res", "g"))
    y, s = OF.ln_shift_res(x, res, g, shift=True)
    torch.autograd.backward([y, s], [cu(inp["dy"]), cu(inp["ds"])])
    got = run_ln(case)
    assert torch.equal(y, got["y"]) and torch.equal(s, got["s"])
    assert torch.equal(x.grad, got["dx"]) and torch.equal(res.grad, got["dx"])
    assert torch.equal(g.grad, got["dw"])


# ---------------------------------------------------------------------------
# glu / gelu
# ---------------------------------------------------------------------------

def run_act(kind, case):
    inp = (K.glu_inputs if kind == "glu" else K.gelu_inputs)(case)
    h, dy = cu(inp["h"]), cu(inp["dy"])
    if kind == "glu":
        return dict(y=C().glu_fwd(h), dh=C().glu_bwd(dy, h))
    return dict(y=C().gelu_fwd(h), dh=C().gelu_bwd(dy, h))


@pytest.mark.parametrize("dn", DTYPES)
@pytest.mark.parametrize("which", range(3), ids=["row_stride", "two_col_blocks",
                                                 "sweep"])
def test_glu_paths(dn, which):
    """4100 narrow rows on 4096 row stripes; a half width of 257/258 vectors
    (two column blocks, the second all tail) over 2050 rows on 2048
    stripes; gates over [-30, 30] with +-0 and the tanh clamp."""
    case = K.glu_cases(K._dt(dn))[which]
    expect("glu", dn, K.act_errors(run_act("glu", case), K.glu_oracle_of(case)),
           case[1:])


@pytest.mark.parametrize("dn", DTYPES)
@pytest.mark.parametrize("which", range(2), ids=["grid_stride", "sweep"])
def test_gelu_paths(dn, which):
    """more than 2048 * 256 vectors, so the stride loop takes a ragged
    second trip; and the value sweep"""
    case = K.gelu_cases(K._dt(dn))[which]
    expect("gelu", dn, K.act_errors(run_act("gelu", case),
                                    K.gelu_oracle_of(case)), case[1:])


def test_glu_gelu_autograd_wiring():
    for kind, fn in (("glu", OF.glu_gelu), ("gelu", OF.gelu)):
        case = (K.glu_cases if kind == "glu" else K.gelu_cases)(K.BF16)[-1]
        inp = (K.glu_inputs if kind == "glu" else K.gelu_inputs)(case)
        h = cu(inp["h"]).requires_grad_(True)
        y = fn(h)
        y.backward(cu(inp["dy"]))
        got = run_act(kind, case)
        assert torch.equal(y, got["y"]) and torch.equal(h.grad, got["dh"])


# ---------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------

def run_ce(case):
    inp = K.ce_inputs(case)
    logits, targets, dnll = (cu(inp[k]) for k in ("logits", "targets", "dnll"))
    nll, lse = C().ce_fwd(logits, targets)
    return dict(nll=nll, lse=lse,
                dlogits=C().ce_bwd(dnll, logits, targets, lse))


@pytest.mark.parametrize("dn", DTYPES)
@pytest.mark.parametrize("V", K.CE_V)
def test_ce_rows(dn, V):
    """nll, lse and dlogits per row: V below, at and above a wave's 64
    lanes, 1 / 5 / 99 rows (one block is 4 rows), targets at 0, V-1 and
    the argmax, and a row with dnll = 0"""
    for case in K.ce_cases(K._dt(dn)):
        if case[1] != "rand" or case[3] != V:
            continue
        got = run_ce(case)
        dead = K.ce_inputs(case)["dnll"] == 0
        assert (got["dlogits"][cu(dead)] == 0).all(), case
        expect("ce", dn, K.ce_errors(got, K.ce_oracle_of(case)), case[1:])


def test_ce_extreme_rows_fp32():
    """one logit at +80 (and at +100) over a floor of -80 (-100), an
    all-equal row, a dead row"""
    case = ("fp32", "extreme", 4, 256)
    got = run_ce(case)
    assert (got["dlogits"][3] == 0).all()
    expect("ce", "fp32", K.ce_errors(got, K.ce_oracle_of(case)), case[1:])


@pytest.mark.parametrize("dn", DTYPES)
def test_ce_masked_mean_wiring(dn):
    """functional.cross_entropy (pad tail, first pad kept as EOS) against
    reference.cross_entropy in fp64: the loss within the per-row nll bound,
    its gradient within the dlogits bound"""
    g = torch.Generator().manual_seed(33)
    B, N, V = 3, 33, 256
    logits = (torch.randn(B, N, V, generator=g) * 3).to(K._dt(dn))
    targets = torch.randint(1, V, (B, N), generator=g)
    targets[:, -5:] = 0
    targets[1, 10:] = 0
    x = cu(logits).requires_grad_(True)
    loss = OF.cross_entropy(x, cu(targets))
    loss.backward()
    x64 = logits.double().requires_grad_(True)
    loss64 = R.cross_entropy(x64, targets)
    loss64.backward()
    errs = dict(nll=K.elem_err(loss, loss64.detach(), floor=1.0),
                dlogits=K.row_err(x.grad, x64.grad))
    dead = cu(x64.grad.abs().amax(-1) == 0)
    assert dead.any() and (x.grad[dead] == 0).all()
    expect("ce", dn, errs, "masked_mean")


# ---------------------------------------------------------------------------
# rope_qkv
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", K.ROPE_SHAPES)
def test_rope_qkv_within_one_ulp(shape):
    """(2, 64, 11): 264 vector units, two column blocks; (3, 704, 2): 2112
    rows on 2048 stripes, positions restarting per batch. Every element
    within one bf16 step of the correctly rounded fp64 rotation."""
    B, N, H = shape
    qkv = K.rope_inputs(shape)
    sin, cos = K.rope_tables(N)
    got = C().rope_qkv(cu(qkv), cu(sin), cu(cos))
    want = K.rope_explicit(qkv.double(), sin.double(), cos.double())
    dist = K.bf16_ulp_dist(got, want)
    print(f"KTOL|rope_qkv|qkv_rot|bf16|ulp 1|ulp 1|ulp {dist}|{shape}")
    assert dist <= 1


# ---------------------------------------------------------------------------
# local attention
# ---------------------------------------------------------------------------

def run_attn(inp):
    qkv, sin, cos, dout = (cu(inp[k]) for k in ("qkv", "sin", "cos", "dout"))
    halo = cu(inp.get("halo"))
    H, wsz = inp["H"], inp["wsz"]
    rot = C().rope_qkv(qkv, sin, cos)
    out, lse = C().attn_fwd(rot, H, wsz, halo=halo)
    res = C().attn_bwd(dout, rot, sin, cos, out, lse, H, wsz, halo=halo)
    got = dict(out=out, lse=lse, dqkv=res[0])
    if halo is not None:
        got["dhalo"] = res[1]
    return got


@pytest.mark.parametrize("case", K.attn_cases(),
                         ids=lambda c: f"{c[0]}-{c[1]}-" + "x".join(map(str, c[2])))
def test_attn_partial_rounds(case):
    """windows of 128, 192 and 320: forward sub-blocks with idle waves,
    backward rounds of 2, 3 and 4 + 1 chunks; near-uniform (1/8) and
    peaked (1.0) logits, and a dominant key met in the first or the last
    key tile. out and dqkv per row and head; lse = max + log(sum) of the
    scaled logits, window 0's zero keys included."""
    inp = K.attn_inputs(case)
    expect("attn", "bf16", K.attn_errors(run_attn(inp), K.attn_oracle_of(case),
                                         inp), f"{case[0]}-{case[1]}-{case[2]}")


def test_attn_halo_against_joined_sequence():
    """second virtual rank at wsz 192: out, dqkv and dhalo against the fp64
    oracle of the joined sequence"""
    inp = K.halo_inputs()["second"]
    expect("attn_halo", "bf16",
           K.attn_errors(run_attn(inp), K.halo_oracle(), inp), K.HALO_SHAPE)


def _band_inputs(wsz):
    B, H, N = 1, 2, 4 * wsz
    g = torch.Generator().manual_seed(50 + wsz)
    qkv = (torch.randn(B, N, 3 * H * 64, generator=g) * 0.5).to(K.BF16)
    sin, cos = K.rope_tables(N)
    return B, H, N, cu(qkv), cu(sin), cu(cos), g


@pytest.mark.parametrize("wsz", [128, 192])
def test_attn_forward_band_is_exact(wsz):
    """k and v of row p reach rows [p, (p // wsz + 2) * wsz) and no other:
    rows outside are bit-identical, every row inside changes"""
    B, H, N, qkv, sin, cos, _ = _band_inputs(wsz)

    def fwd(x):
        return C().attn_fwd(C().rope_qkv(x, sin, cos), H, wsz)[0]

    base = fwd(qkv)
    for p in (wsz - 1, wsz, 2 * wsz - 1):
        x = qkv.clone()
        x[:, p, H * 64:] += 1.0
        changed = (fwd(x) != base).any(dim=-1)[0].cpu()
        lo, hi = p, (p // wsz + 2) * wsz
        assert not changed[:lo].any() and not changed[hi:].any(), p
        assert changed[lo:hi].all(), p


@pytest.mark.parametrize("wsz", [128, 192])
def test_attn_backward_band_is_exact(wsz):
    """dout at row i alone: dq is zero off row i, dk and dv are exactly
    zero outside [(i // wsz - 1) * wsz, i] and non-zero on every row inside"""
    B, H, N, qkv, sin, cos, g = _band_inputs(wsz)
    rot = C().rope_qkv(qkv, sin, cos)
    out, lse = C().attn_fwd(rot, H, wsz)
    for i in (wsz - 1, wsz, 2 * wsz - 1):
        dout = torch.zeros_like(out)
        dout[:, i] = cu(torch.randn(H * 64, generator=g).to(K.BF16))
        dqkv = C().attn_bwd(dout, rot, sin, cos, out, lse, H, wsz)[0][0].cpu()
        dq, dkv = dqkv[:, :H * 64], dqkv[:, H * 64:]
        live_q = (dq != 0).any(dim=-1)
        assert live_q[i] and live_q.sum() == 1, i
        live = (dkv != 0).any(dim=-1)
        lo = max(0, (i // wsz - 1) * wsz)
        assert not live[:lo].any() and not live[i + 1:].any(), i
        assert live[lo:i + 1].all(), i


def test_attn_autograd_wiring():
    inp = K.attn_inputs(("rand", 1.0, (1, 192, 2, 192)))
    qkv = cu(inp["qkv"]).requires_grad_(True)
    out = OF.local_attention(qkv, cu(inp["sin"]), cu(inp["cos"]), 2, 192)
    out.backward(cu(inp["dout"]))
    got = run_attn(inp)
    assert torch.equal(out, got["out"]) and torch.equal(qkv.grad, got["dqkv"])


# ---------------------------------------------------------------------------
# SGU
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", K.SGU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sgu_kernels_direct(shape):
    """N = 512 / 768: row blocks past the first (ktiles and my_kmax of
    sgu_fwd for mblk >= 1, mstart > 0 of sgu_dgate); D = 832: the second,
    64-channel dW chunk. W ~ N^-0.5 with a full upper triangle, which must
    leave no trace: dW's upper triangle is exactly zero."""
    B, N, D = shape
    inp = {k: cu(v) for k, v in K.sgu_inputs(shape)["direct"].items()}
    out, gate_out = C().sgu_fwd(inp["xa"], inp["g_ln"], inp["w"], inp["bias"])
    dg = C().sgu_dgate(inp["t"], inp["w"])
    dw = C().sgu_dw(inp["t"], inp["g_ln"], *OF._tri_tiles(N, inp["t"].device))
    assert (dw.triu(1) == 0).all()
    expect("sgu_direct", "bf16",
           K.sgu_direct_errors(dict(out=out, gate_out=gate_out, dg=dg, dw=dw),
                               K.sgu_direct_oracle_of(shape)), shape)


def run_sgu_e2e(shape):
    inp = K.sgu_inputs(shape)["e2e"]
    x, gw, w, bias = (cu(inp[k]).requires_grad_(True)
                      for k in ("x", "gw", "w", "bias"))
    out = OF.sgu_gate(x, gw, w, bias)
    out.backward(cu(inp["dy"]))
    d2 = shape[2]
    assert (w.grad.triu(1) == 0).all()
    return dict(out=out.detach(), dxa=x.grad[..., :d2], dgate=x.grad[..., d2:],
                dgw=gw.grad, dW=w.grad, db=bias.grad)


@pytest.mark.parametrize("shape", K.SGU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sgu_gate_end_to_end(shape):
    """functional.sgu_gate forward and backward; the gate half and the xa
    half of x.grad each on its own scale"""
    expect("sgu_e2e", "bf16",
           K.sgu_e2e_errors(run_sgu_e2e(shape), K.sgu_e2e_oracle_of(shape)),
           shape)


def test_sgu_composite_fallback():
    """N = 128 takes the library-matmul path; same oracle"""
    s = K.SGU_COMPOSITE_SHAPE
    expect("sgu_composite", "bf16",
           K.sgu_e2e_errors(run_sgu_e2e(s), K.sgu_e2e_oracle_of(s)), s)


@pytest.mark.parametrize("p", [255, 256, 300])
def test_sgu_causality_across_row_blocks(p):
    """a change at row p of a 512-row sequence leaves every earlier row
    bit-identical and changes row p and the later ones (all but the few
    whose W[m, p] is too small to move a bf16 output)"""
    inp = K.sgu_inputs((2, 512, 64))["e2e"]
    x, gw, w, bias = (cu(inp[k]) for k in ("x", "gw", "w", "bias"))
    base = OF.sgu_gate(x, gw, w, bias)
    x2 = x.clone()
    x2[0, p] += 1.0
    changed = (OF.sgu_gate(x2, gw, w, bias) != base).any(dim=-1).cpu()
    assert not changed[0, :p].any() and not changed[1].any()
    assert changed[0, p] and changed[0, p:].float().mean() > 0.8


# ---------------------------------------------------------------------------
# fused_adamw / grad_sumsq
# ---------------------------------------------------------------------------

def run_adamw(dn, sharded):
    inp = K.adamw_inputs(dn, sharded)
    lo, hi = inp["lo"], inp["hi"]
    state = {k: cu(inp[k][lo:hi].clone())
             for k in ("master", "exp_avg", "exp_avg_sq")}
    params = cu(inp["params"].clone())
    starts, ends, decay = cu(inp["starts"]), cu(inp["ends"]), cu(inp["decay"])
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    clip = torch.full((1,), K.ADAMW_CLIP, device=DEV)
    hp = K.ADAMW_HP
    for grads in inp["grads"]:
        C().fused_adamw(state["master"], params, cu(grads), state["exp_avg"],
                        state["exp_avg_sq"], starts, ends, decay, hp["lr"],
                        hp["b1"], hp["b2"], hp["eps"], hp["wd"], step,
                        K.ADAMW_GRAD_SCALE, clip, shard_off=lo)
    assert int(step.item()) == K.ADAMW_STEPS
    got = dict(params=params.cpu())
    for k, v in state.items():
        full = inp[k].clone()
        full[lo:hi] = v.cpu()
        got[k] = full
    return inp, got


@pytest.mark.parametrize("dn", DTYPES)
@pytest.mark.parametrize("sharded", [False, True], ids=["full", "shard_off"])
def test_fused_adamw_formula(dn, sharded):
    """2100 ragged chunks on 2048 blocks (lengths 0, 1, 24, 257, ...), mixed
    decay flags, grad_scale 0.25, clip 0.5, three steps from step 1, params
    in bf16 and in fp32, the whole space and a shard starting inside a
    chunk: master, both moments and params against the fp64 formula, and
    whatever no chunk covers left as it was"""
    inp, got = run_adamw(dn, sharded)
    cov = torch.zeros(inp["P"], dtype=torch.bool)
    for s, e in zip(inp["starts"].tolist(), inp["ends"].tolist()):
        cov[s:e] = True
    for k in ("master", "exp_avg", "exp_avg_sq"):
        assert torch.equal(got[k][~cov], inp[k][~cov]), k
    assert torch.equal(got["params"][~cov], inp["params"][~cov])
    expect("adamw", dn, K.adamw_errors(got, K.adamw_oracle_of(dn, sharded), inp),
           "shard_off" if sharded else "full")


@pytest.mark.parametrize("dn", DTYPES)
@pytest.mark.parametrize("numel", K.SUMSQ_NUMEL)
def test_grad_sumsq(dn, numel):
    """one vector, and three vectors more than 2048 blocks cover in a trip"""
    x = K.sumsq_inputs(dn, numel)
    got = C().grad_sumsq(cu(x))
    expect("sumsq", dn, dict(sumsq=K.elem_err(got, K.sumsq_oracle(x))), numel)


# ---------------------------------------------------------------------------
# fp8 quantization
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", K.FP8_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fp8_quantize_bytes(shape):
    """ragged 64 x 64 tiles of the transposing kernel, values beyond
    +-448 * scale, zeros of both signs and e4m3 subnormals: the bytes of
    clamp(t * (1 / scale)) exactly. The flat kernel wants numel % 8 == 0,
    which (66, 70) is not."""
    t, scale = K.fp8_inputs(shape)
    want = K.fp8_reference(t, scale)
    runs = [("t", C().fp8_quantize_t(cu(t), cu(scale)), want.t())]
    if t.numel() % 8 == 0:
        runs.append(("flat", C().fp8_quantize(cu(t), cu(scale)), want))
    div = K.fp8_reference(t, scale, divide=True)
    for name, got, ref in runs:
        got = got.view(torch.uint8).cpu()
        assert got.shape == ref.shape
        bad = (got != ref).sum().item()
        if bad:   # which inputs, as value / scale, kernel byte, reference byte
            src = (t.float() / scale).t() if name == "t" else t.float() / scale
            at = (got != ref).nonzero()[:8]
            print("fp8 differs:", [(src[tuple(i)].item(), got[tuple(i)].item(),
                                    ref[tuple(i)].item()) for i in at])
        vs_div = (got != (div.t() if name == "t" else div)).float().mean().item()
        print(f"KTOL|fp8_quantize_{name}|bytes|e4m3|exact|0 differ|{bad} differ"
              f"|{shape}, {vs_div:.2%} differ from the divide form")
        assert bad == 0, (name, shape, bad)
