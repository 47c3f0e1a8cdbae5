"""CPU proof that the comparator of tests/kernel_oracle.py discriminates.

For every family of cases in tests/test_gpu_kernel_edges.py: the explicit
formulas agree with progen_amd/ops/reference.py in fp64, the bf16/fp32
emulation of the kernel passes the family's bound, and every mutant — the
same formulas with one defect a kernel could plausibly have — misses it.
A mutant that passed would mean the GPU test cannot see that defect.
"""

import math

import pytest
import torch

import kernel_oracle as K

BF16, F32, F64 = K.BF16, K.F32, K.F64
DTYPES = ["bf16", "fp32"]


def missed(family, dn, errs):
    b = K.bounds(family, dn)
    return [k for k, v in errs.items() if not v <= b[k][1]]


def same64(a, b, tol=1e-9):
    for k in b:
        if k in a:
            assert K.row_err(a[k], b[k]) < tol, k


# ---------------------------------------------------------------------------
# the comparator itself
# ---------------------------------------------------------------------------

def test_row_err_quiet_row_cannot_hide():
    want = torch.tensor([[100.0, -50.0], [1.0, 0.5]])
    got = want.clone()
    got[1, 0] = 1.1   # 10 % of its own row, 0.1 % of the loudest element
    assert K.row_err(got, want, floor=0.0) == pytest.approx(0.1)
    # the default floor is 1/64 of the loudest element: 0.1 / (100/64)
    assert K.row_err(got, want) == pytest.approx(0.1 * 64 / 100)
    got[0, 0] = float("nan")
    assert K.row_err(got, want) == math.inf


def test_elem_err_and_ulp_distance():
    want = torch.tensor([1.0, 10.0])
    assert K.elem_err(torch.tensor([1.01, 10.0]), want) == pytest.approx(0.01)
    x = torch.tensor([1.0, -1.0, 0.0, 3.0], dtype=BF16)
    assert K.bf16_ulp_dist(x, x.double()) == 0
    up = torch.tensor([1.0 + 2 ** -7, -1.0, -0.0, 3.0], dtype=BF16)
    assert K.bf16_ulp_dist(up, x.double()) == 1
    assert K.bf16_ulp_dist(torch.tensor([2 ** -133], dtype=BF16),
                           torch.tensor([-2.0 ** -133], dtype=F64)) == 2


# ---------------------------------------------------------------------------
# ln_shift
# ---------------------------------------------------------------------------

def _ln_case(dn, shape, variant, offset=0.0):
    return (dn, *shape, *variant, offset)


@pytest.mark.parametrize("variant", K.LN_VARIANTS)
def test_ln_explicit_is_the_reference(variant):
    case = _ln_case("fp32", (3, 2, 48), variant)
    same64(K.ln_emulate(case, dt=F64), K.ln_oracle_of(case))


@pytest.mark.parametrize("dn", DTYPES)
def test_ln_emulation_passes_mutants_fail(dn):
    for case in K.ln_cases(K._dt(dn)):
        errs = K.ln_errors(K.ln_emulate(case), K.ln_oracle_of(case), case)
        assert not missed(K.ln_family(case), dn, errs), case
    for variant in [(True, True, True), (True, False, False)]:
        for shape in [(2, 32, 128), (3, 2, 48), (3, 345, 32)]:
            case = _ln_case(dn, shape, variant)
            for mutant in ("shift_same_row", "shift_cross_batch",
                           "last_row_grad_kept"):
                errs = K.ln_errors(K.ln_emulate(case, mutant),
                                   K.ln_oracle_of(case), case)
                assert missed(K.ln_family(case), dn, errs), (mutant, case)
    # the one-pass variance, in the fp32 arithmetic the kernel uses, on the
    # rows with mean 10. ln_shift: the statistics miss in both dtypes and y
    # in fp32. ln_shift_res: in fp32; in bf16 the rounding of s = x + res
    # moves rstd by more than the one-pass form does, so nothing can show.
    plain, res = K.ln_cases(K._dt(dn))[-2:]
    assert plain[-1] == res[-1] == 10.0 and res[5] and not plain[5]
    errs = K.ln_errors(K.ln_emulate(plain, "one_pass_var"),
                       K.ln_oracle_of(plain), plain)
    assert "rstd" in missed("ln", dn, errs)
    if dn == "fp32":
        assert "y" in missed("ln", dn, errs)
        errs = K.ln_errors(K.ln_emulate(res, "one_pass_var"),
                           K.ln_oracle_of(res), res)
        assert {"rstd", "y"} <= set(missed("ln_res", dn, errs))


# ---------------------------------------------------------------------------
# glu / gelu
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dn", DTYPES)
def test_act_emulation_passes_mutants_fail(dn):
    for kind, cases, oracle_of in (
            ("glu", K.glu_cases(K._dt(dn)), K.glu_oracle_of),
            ("gelu", K.gelu_cases(K._dt(dn)), K.gelu_oracle_of)):
        sweep = [c for c in cases if c[1] == "sweep"][0]
        same64(K.act_emulate(kind, sweep, dt=F64), oracle_of(sweep))
        for c in cases:
            errs = K.act_errors(K.act_emulate(kind, c), oracle_of(c))
            assert not missed(kind, dn, errs), c
        # erf-GELU is within 5e-4 of the tanh form: below bf16 storage
        mutants = ["no_clamp"] + ["halves_swapped"] * (kind == "glu") + \
            ["erf"] * (dn == "fp32")
        for mutant in mutants:
            errs = K.act_errors(K.act_emulate(kind, sweep, mutant),
                                oracle_of(sweep))
            assert missed(kind, dn, errs), (kind, mutant)


# ---------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dn", DTYPES)
def test_ce_emulation_passes_mutants_fail(dn):
    for c in K.ce_cases(K._dt(dn)):
        same64(K.ce_emulate(c, dt=F64) if dn == "fp32" else {}, K.ce_oracle_of(c))
        errs = K.ce_errors(K.ce_emulate(c), K.ce_oracle_of(c))
        assert not missed("ce", dn, errs), c
        if c[3] > 1:
            errs = K.ce_errors(K.ce_emulate(c, "onehot_plus1"), K.ce_oracle_of(c))
            assert "dlogits" in missed("ce", dn, errs), c
    if dn == "fp32":
        c = ("fp32", "extreme", 4, 256)
        errs = K.ce_errors(K.ce_emulate(c, "no_max_sub"), K.ce_oracle_of(c))
        assert {"nll", "lse"} <= set(missed("ce", dn, errs))


# ---------------------------------------------------------------------------
# rope_qkv
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", K.ROPE_SHAPES)
def test_rope_emulation_within_one_ulp_mutant_not(shape):
    B, N, H = shape
    qkv = K.rope_inputs(shape)
    sin, cos = K.rope_tables(B * N)
    want = K.rope_explicit(qkv.double(), sin.double(), cos.double())
    # the explicit form is reference.apply_rotary_pos_emb per head
    x = qkv.double().reshape(B, N, 3 * H, 64).transpose(1, 2)
    ref = K.R.apply_rotary_pos_emb(x, sin[:N].double(), cos[:N].double())
    assert torch.equal(ref.transpose(1, 2).reshape(B, N, -1), want)
    emu = K.rope_explicit(qkv.float(), sin, cos).to(BF16)
    assert K.bf16_ulp_dist(emu, want) <= 1
    if B > 1:
        bad = K.rope_explicit(qkv.float(), sin, cos, mutant="pos_bn").to(BF16)
        assert K.bf16_ulp_dist(bad, want) > 1


# ---------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------

ATTN_MUTANTS = ("mask_minus1", "mask_plus1", "oldest_dropped",
                "no_zero_quirk", "v_not_rotated")


# where a defect changes nothing a bound could see; every other (mutant,
# case) pair must miss
ATTN_BLIND = {
    # one window: the oldest lookback key is one of 192 identical zero keys
    ("oldest_dropped", "rand", (1, 192, 2, 192)),
    # the extra key of a mask one too wide is drowned by the hot key, which
    # sits at offset 0 and is visible to every row either way; the same
    # shape catches the defect in the hot_last and rand cases
    ("mask_plus1", "hot_first", (1, 384, 2, 192)),
}


def test_attn_explicit_is_the_reference():
    inp = K.attn_inputs(("rand", 1.0, (2, 256, 3, 128)))
    ex = K.attn_emulate(inp, dt=F64)
    same64(ex, K.attn_oracle(**inp))
    # lse: logsumexp of the scaled logits, the zero keys of window 0
    # included — row 0 sees 128 of them and itself
    q = K.attn_explicit(inp["qkv"].double(), inp["sin"].double(),
                        inp["cos"].double(), inp["dout"].double(), 3, 128)
    assert q["lse"].shape == (2, 3, 256)
    assert (q["lse"][:, :, 0] > math.log(128)).all() or \
        (q["lse"][:, :, 0] > 0).all()


def test_attn_halo_oracle_is_the_joined_sequence():
    """out, dqkv and dhalo of the second rank, with the exact rotated k|v
    of the first rank's last window as halo, are the joined sequence's."""
    h = K.halo_inputs()
    j, s = h["joined"], h["second"]
    B, N, H, wsz = K.HALO_SHAPE
    L = N // 2
    x = j["qkv"].double().requires_grad_(True)
    sin, cos = j["sin"].double(), j["cos"].double()
    out = K.R.local_attention(x, sin, cos, H, wsz)
    dout = j["dout"].double().clone()
    dout[:, :L] = 0      # only the second rank's rows send gradient back
    out.backward(dout)
    tail = x.detach()[:, L - wsz:L].reshape(B, wsz, 3 * H, 64)[:, :, H:]
    sw, cw = sin[L - wsz:L].reshape(1, wsz, 1, 64), cos[L - wsz:L].reshape(1, wsz, 1, 64)
    halo = (tail * cw + K.R.rotate_every_two(tail) * sw).reshape(B, wsz, -1)
    ex = K.attn_explicit(s["qkv"].double(), s["sin"].double(), s["cos"].double(),
                         s["dout"].double(), H, wsz, halo=halo)
    assert K.row_err(ex["out"], out.detach()[:, L:]) < 1e-9
    assert K.row_err(ex["dqkv"], x.grad[:, L:]) < 1e-9
    # dhalo lives in rotated space: rotate it back onto the first rank's k|v
    dh = ex["dhalo"].reshape(B, wsz, 2 * H, 64)
    back = K._inv_rot(dh, sw, cw).reshape(B, wsz, 2 * H * 64)
    assert K.row_err(back, x.grad[:, L - wsz:L, H * 64:]) < 1e-9


def test_attn_emulation_passes_mutants_fail():
    for c in K.attn_cases():
        inp = K.attn_inputs(c)
        errs = K.attn_errors(K.attn_emulate(inp), K.attn_oracle_of(c), inp)
        assert not missed("attn", "bf16", errs), c
        for mutant in ATTN_MUTANTS:
            if (mutant, c[0], c[2]) in ATTN_BLIND:
                continue
            errs = K.attn_errors(K.attn_emulate(inp, mutant),
                                 K.attn_oracle_of(c), inp)
            assert missed("attn", "bf16", errs), (mutant, c)
    inp = K.halo_inputs()["second"]
    errs = K.attn_errors(K.attn_emulate(inp), K.halo_oracle(), inp)
    assert not missed("attn_halo", "bf16", errs)
    for mutant in ("mask_minus1", "mask_plus1", "oldest_dropped",
                   "v_not_rotated"):
        errs = K.attn_errors(K.attn_emulate(inp, mutant), K.halo_oracle(), inp)
        assert missed("attn_halo", "bf16", errs), mutant


def test_attn_inputs_are_peaked_where_they_claim():
    """the hot-key cases put most of a row's weight on one key"""
    for kind in ("hot_first", "hot_last"):
        inp = K.attn_inputs((kind, 0.125, (1, 384, 2, 192)))
        wsz = inp["wsz"]
        o = K.attn_oracle_of((kind, 0.125, (1, 384, 2, 192)))
        # a row that sees hot keys: lse is about the hot logit, far above
        # the log(number of keys) of a flat softmax
        row = 2 * wsz - 1
        assert (o["lse"][:, :, row] > math.log(2 * wsz) + 1).all(), kind


# ---------------------------------------------------------------------------
# SGU
# ---------------------------------------------------------------------------

SGU_MUTANTS = ("tril_minus1", "tril_plus1", "no_bias", "skip_ktile",
               "dw_first_chunk_only")


def test_sgu_explicit_is_the_reference():
    shape = (2, 512, 64)
    same64(K.sgu_e2e_emulate(shape, dt=F64), K.sgu_e2e_oracle_of(shape))


def test_sgu_emulation_passes_mutants_fail():
    for shape in K.SGU_SHAPES:
        errs = K.sgu_direct_errors(K.sgu_direct_emulate(shape),
                                   K.sgu_direct_oracle_of(shape))
        assert not missed("sgu_direct", "bf16", errs), shape
        errs = K.sgu_e2e_errors(K.sgu_e2e_emulate(shape),
                                K.sgu_e2e_oracle_of(shape))
        assert not missed("sgu_e2e", "bf16", errs), shape
    for mutant in SGU_MUTANTS:
        # the K-tile defect needs rows >= 256, the dW one channels >= 768
        shape = (2, 512, 832)
        d = missed("sgu_direct", "bf16", K.sgu_direct_errors(
            K.sgu_direct_emulate(shape, mutant), K.sgu_direct_oracle_of(shape)))
        e = missed("sgu_e2e", "bf16", K.sgu_e2e_errors(
            K.sgu_e2e_emulate(shape, mutant), K.sgu_e2e_oracle_of(shape)))
        assert d and e, (mutant, d, e)
        if mutant.startswith("tril"):
            assert {"out", "gate_out", "dg"} <= set(d), (mutant, d)
            assert {"out", "dgate"} <= set(e), (mutant, e)
    s = K.SGU_COMPOSITE_SHAPE
    errs = K.sgu_e2e_errors(K.sgu_e2e_emulate(s, composite=True),
                            K.sgu_e2e_oracle_of(s))
    assert not missed("sgu_composite", "bf16", errs)
    for mutant in ("tril_minus1", "tril_plus1", "no_bias"):
        errs = K.sgu_e2e_errors(K.sgu_e2e_emulate(s, mutant, composite=True),
                                K.sgu_e2e_oracle_of(s))
        assert missed("sgu_composite", "bf16", errs), mutant


def test_old_sgu_inputs_hide_the_diagonal_new_ones_do_not():
    """W ~ 1e-3 with bias 1 lets a tril(-1) matmul through the whole-tensor
    metric of tests/test_gpu_kernels.py; W ~ N^-0.5 with a random bias does
    not let it through row_err."""
    g = torch.Generator().manual_seed(11)
    B, N, D = 2, 256, 128
    x = (torch.randn(B, N, 2 * D, generator=g) / 4).to(BF16).double()
    gw = torch.randn(D, generator=g).to(BF16).double()
    W = (torch.randn(N, N, generator=g) * 1e-3).to(BF16).double()
    b = torch.ones(N, 1, dtype=F64)
    dy = (torch.randn(B, N, D, generator=g) / 4).to(BF16).double()
    good = K.sgu_e2e_explicit(x, gw, W, b, dy)
    bad = K.sgu_e2e_explicit(x, gw, W, b, dy, mutant="tril_minus1")
    whole = ((bad["out"] - good["out"]).abs().max() / good["out"].abs().max())
    assert whole < 2e-2    # the old inputs and metric pass the mutant
    shape = (2, 512, 64)
    new = K.sgu_e2e_errors(K.sgu_e2e_emulate(shape, "tril_minus1"),
                           K.sgu_e2e_oracle_of(shape))
    assert new["out"] > 0.2 and new["dgate"] > 0.1


# ---------------------------------------------------------------------------
# AdamW / grad_sumsq
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dn", DTYPES)
def test_adamw_emulation_passes_mutants_fail(dn):
    for sharded in (False, True):
        inp = K.adamw_inputs(dn, sharded)
        errs = K.adamw_errors(K.adamw_emulate(dn, sharded),
                              K.adamw_oracle_of(dn, sharded), inp)
        assert not missed("adamw", dn, errs), sharded
        for mutant in ("no_bias_correction", "decay_everywhere",
                       "grad_scale_ignored"):
            errs = K.adamw_errors(K.adamw_emulate(dn, sharded, mutant),
                                  K.adamw_oracle_of(dn, sharded), inp)
            assert "master" in missed("adamw", dn, errs), (mutant, sharded)
    # elements outside every chunk are left alone
    inp = K.adamw_inputs(dn, False)
    cov = torch.zeros(inp["P"], dtype=torch.bool)
    for s, e in zip(inp["starts"].tolist(), inp["ends"].tolist()):
        cov[s:e] = True
    assert (~cov).sum() > 100
    o = K.adamw_oracle_of(dn, False)
    assert torch.equal(o["master"][~cov], inp["master"].double()[~cov])
    lens = set((inp["ends"] - inp["starts"]).tolist())
    assert {0, 1, 24, 257} <= lens and len(inp["starts"]) == 2100


@pytest.mark.parametrize("dn", DTYPES)
def test_sumsq_emulation_passes_mutant_fails(dn):
    b = K.bounds("sumsq", dn)["sumsq"][1]
    for n in K.SUMSQ_NUMEL:
        x = K.sumsq_inputs(dn, n)
        want = K.sumsq_oracle(x)
        assert K.elem_err(K.sumsq_emulate(x), want) <= b
        # a grid-stride loop that never takes its second trip
        vlen = 8 if dn == "bf16" else 4
        first = min(x.numel(), 2048 * 256 * vlen)
        if first < x.numel():
            assert K.elem_err(K.sumsq_oracle(x[:first]), want) > b


# ---------------------------------------------------------------------------
# fp8 reference
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", K.FP8_SHAPES)
def test_fp8_inputs_cover_their_classes(shape):
    t, scale = K.fp8_inputs(shape)
    y = t.float() / scale
    assert (y.abs() > 448).any() and (y == 0).any()
    assert ((y.abs() > 0) & (y.abs() < 2 ** -6)).any()      # e4m3 subnormals
    q = K.fp8_reference(t, scale)
    assert q.shape == shape and q.dtype == torch.uint8
    # saturation, not NaN: 0x7e / 0xfe are +-448
    assert ((q & 0x7F) != 0x7F).all()
    assert (q[y > 448] == 0x7E).all() and (q[y < -448] == 0xFE).all()
