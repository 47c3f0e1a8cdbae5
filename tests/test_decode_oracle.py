"""CPU proof that the bounds of tests/decode_oracle.py discriminate.

For each family of the decode-step kernels (``dec_ln``, ``dec_ln_res``,
``dec_attn``, ``dec_sgu``) and each dtype: the explicit formulas agree with
progen_amd/ops/reference.py in fp64; the emulation's error is above zero
and, by construction, within the bound; the bound is tighter than the old
global tolerance of tests/test_gpu_decode_fused.py; and every mutant misses
the bound on at least one output at every case it applies to, of which
there are at least three. A mutant that passed would mean that
tests/test_gpu_decode_kernel_edges.py cannot see that defect.

Applicable sets narrower than the kernel's branch alone, all chosen from the
inputs and none from a result:
  - ``no_scale``, the zero-lookback mutants and ``current_row_left_out``
    take the plain ``randn`` family only: against a peaked logit of 144 a
    logit of 0 or of the current row weighs nothing in any precision, and
    a one-hot softmax stays one-hot without the scale;
  - ``band_starts_at_w0`` leaves out ``peak_last``, whose peak lies in the
    current window; ``v_not_rotated`` leaves out position 0, where the
    rotation is the identity;
  - ``empty_unguarded`` stands for the issue's "an empty group combined
    with weight 1", which computes the same values (an empty group's sums
    are 0): see ``ATTN_MUTANTS``;
  - ``zero_count_minus1`` in bf16 takes window 64 with at most 8 cached
    rows, where one zero key is 1/72 of the mass or more;
  - ``last_row_dropped`` of ``dec_attn`` leaves out the ``peak_first``
    family, whose peak at the band's first row outweighs the lost row,
    unless the band has one row;
  - the ``dec_sgu`` mutants that lose one term take the cases whose lost
    weight or bias is at least half its standard deviation;
  - ``stats_short`` (D <= 128) leaves out D = 128 with a residual in bf16:
    that family's bound is set by the rounded sum at D = 16, and 8 of 128
    elements move the statistics by less.
"""

import pytest
import torch

import decode_oracle as O
import kernel_oracle as K

DTYPES = ["bf16", "fp32"]
OLD_TOL = {"bf16": 2e-2, "fp32": 1e-5}


def applicable(family, dn, name):
    pred = O.MUTANTS[family][name]
    cases = [c for c in O.family_cases(family, dn) if pred(c)]
    if name == "stats_short" and family == "dec_ln_res" and dn == "bf16":
        cases = [c for c in cases if c[2] == 16]
    if name == "last_row_dropped" and family == "dec_attn":
        cases += [c for c in O.family_cases(family, dn)
                  if c[1] == "peak_first" and O.band(c[2], c[4])[1] == 1]
    return cases


# ---------------------------------------------------------------------------
# the explicit formulas are the reference
# ---------------------------------------------------------------------------

def same64(a, b, tol=1e-9):
    for k in b:
        if b[k] is not None:
            assert K.row_err(a[k], b[k]) < tol, k


@pytest.mark.parametrize("family", O.FAMILIES)
def test_explicit_formulas_are_the_reference_in_fp64(family):
    emulate, oracle, _ = O._parts(family)
    for case in O.family_cases(family, "fp32"):
        if case[2] in (2064, 4096, 2112):      # the widths add nothing here
            continue
        same64(emulate(case, dt=K.F64), oracle(case))


# ---------------------------------------------------------------------------
# the emulation passes, the mutants miss
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dn", DTYPES)
@pytest.mark.parametrize("family", O.FAMILIES)
def test_emulation_passes_and_mutants_miss_the_bound(family, dn):
    b = O.bounds(family, dn)
    for k, (emu, bnd) in b.items():
        print(f"KTOL|{family}|{k}|{dn}|{emu:.3e}|{bnd:.3e}|emulation")
        if k == "kv_ulp":
            # rope_qkv's rule, not a margin: fp32 products rounded once
            # land on the correctly rounded value or next to it
            assert emu <= bnd == 1
            continue
        assert 0 < emu <= bnd, k
        if family == "dec_ln_res" and dn == "bf16":
            # the rounded h + res at D = 16 sets it, as it does for the
            # training kernel: below that table row's bound
            assert bnd < K.bounds("ln_res", "bf16")["y"][1], k
        else:
            assert bnd < OLD_TOL[dn], k
    for name in O.MUTANTS[family]:
        hit = applicable(family, dn, name)
        if name == "h_not_updated" and family == "dec_ln":
            assert not hit                     # no residual, nothing to store
            continue
        assert len(hit) >= 3, (name, len(hit))
        for case in hit:
            errs = O.errors(family, case, mutant=name)
            assert O.misses(family, dn, errs), (name, case, errs, b)


def test_written_attention_rows_round_as_rope_qkv_does():
    """bf16: the emulation's k and v rows are within one bf16 step of the
    correctly rounded fp64 rotation, and an unrotated v is not"""
    for case in O.attn_cases(K.BF16):
        want = O.attn_oracle(case)
        assert O.attn_row_ulps(O.attn_emulate(case), want) <= 1, case
    case = ("bf16", "rand", 64, 256, 33)
    assert O.attn_row_ulps(O.attn_emulate(case, "v_not_rotated"),
                           O.attn_oracle(case)) > 1


def test_every_branch_point_of_the_issue_is_a_case():
    """band lengths with empty groups and around one unrolled round, both
    sides of the ONE boundary, a statistics loop with two chunks a thread"""
    nrows = {O.band(c[2], c[4])[1] for c in O.attn_cases(K.F32)}
    assert {0, 1, 7, 8, 9, 31, 32, 33, 127, 128, 129} <= nrows
    assert O.ATTN_B != O.ATTN_H
    assert {2048, 2064, 16} <= set(O.LN_D)
    assert any(d2 // 8 > 256 for _, d2 in O.SGU_SHAPES)
    assert any(N & (N - 1) for N, _ in O.SGU_SHAPES)
    for dn in DTYPES:
        for c in O.sgu_cases(O._dt(dn)):
            assert 0 <= c[3] < c[1]
        for c in O.attn_cases(O._dt(dn)):
            assert 0 <= c[4] < c[3]


def test_nan_rows_are_where_a_step_must_not_read():
    case = ("bf16", "rand", 64, 256, 191)
    k = O.attn_inputs(case)["k_cache"]
    finite = torch.isfinite(k).all(-1).all(0).all(0)
    assert finite.nonzero().flatten().tolist() == list(range(64, 191))
    h = O.sgu_inputs(("bf16", 192, 192, 33))["hist"]
    finite = torch.isfinite(h).all(-1).all(0)
    assert finite.nonzero().flatten().tolist() == list(range(33))
