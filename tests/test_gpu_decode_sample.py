"""GPU: the decode sampling kernel (progen_amd/ops/hip/decode_sample.hip)
against ``reference.decode_sample``, and the decode loop with the sampler
inside the captured step.

Kernel cases: seeds {1, 2} x (V, k) x B in {1, 3, 32} x {bf16, fp32} x pos
in {0, 5, L - 2} x the logit families of tests/decode_sample_cases.py
(normal, forced ties, all selected scores negative) plus k = 1 at every V.
The uniforms must match bit for bit, greedy tokens and every in-place
effect exactly, and stochastic tokens exactly except at NEAR-TIES.

A near-tie is a row whose best score, evaluated in fp64, leads the largest
score strictly below it by less than 1e-4. Scores stay under 64 in
magnitude, where one fp32 ulp is 3.8e-6; two logs and two adds leave at
most about 3 ulp on each of the two scores, and 1e-4 is four times that.
Exact ties are resolved by index on both sides and are not near-ties. At
most 1 % of the cases may be near-ties: asserted before anything is
compared.
"""

import pytest
import torch

import decode_sample_cases as C
from progen_amd.ops import functional as OF
from progen_amd.ops import reference as R

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs MI355X")]

L = 16
SEEDS = (1, 2)
VK = [(256, 25), (256, 0), (320, 25), (1024, 25), (255, 3), (2, 1)]
BS = (1, 3, 32)
POSITIONS = (0, 5, L - 2)
NEAR_TIE = 1e-4


def _state(B, seed):
    """Sampler state with both branches of every effect in it: tokens in
    {0, 1, 2} (pads to count), odd rows primed to a length that covers
    some of the positions."""
    g = torch.Generator().manual_seed(B)
    seq = torch.randint(0, 3, (B, L), generator=g)
    lens = torch.tensor([0 if b % 2 == 0 else (5 * b) % L for b in range(B)])
    pads = torch.randint(0, 2, (B,), generator=g)
    token = torch.full((B,), -1, dtype=torch.long)
    return [torch.tensor([seed]), seq, lens, pads, token]


def _run(fn, t, pos, st, k, greedy, device):
    """One call on copies of the state ``st``; returns (seq, pads, token, u)
    on the host."""
    seed_t, seq, lens, pads, token = [x.clone().to(device) for x in st]
    u = torch.full(t.shape, -1.0, dtype=torch.float32, device=device)
    fn(t.to(device), torch.tensor(pos).to(device), seed_t, seq, lens, pads,
       token, k, greedy, u)
    return [x.cpu() for x in (seq, pads, token, u)]


def _cases(V, k):
    for seed in SEEDS:
        for B in BS:
            for pos in POSITIONS:
                for fam in C.FAMILIES:
                    yield seed, B, pos, fam, k
                if k != 1:
                    yield seed, B, pos, "normal", 1


@pytest.mark.parametrize("V,k", VK, ids=[f"V{v}-k{k}" for v, k in VK])
def test_kernel_matches_reference(V, k):
    near = total = 0
    checks = []
    for seed, B, pos, fam, kk in _cases(V, k):
        t = C.make_logits(fam, B, V, kk, seed)
        st = _state(B, seed)
        want = _run(R.decode_sample, t, pos, st, kk, False, "cpu")
        want_greedy = _run(R.decode_sample, t, pos, st, kk, True, "cpu")
        exact = C.gap64(t, want[3], kk) >= NEAR_TIE
        near += int((~exact).sum())
        total += B
        for dtype in (torch.bfloat16, torch.float32):
            got = _run(OF.decode_sample, t.to(dtype), pos, st, kk, False,
                       "cuda")
            got_greedy = _run(OF.decode_sample, t.to(dtype), pos, st, kk,
                              True, "cuda")
            checks.append(((seed, B, pos, fam, kk, dtype), exact, want, got,
                           want_greedy, got_greedy))
    print(f"NEARTIE|V={V}|k={k}|rows={total}|near_ties={near}")
    assert near <= 0.01 * total, (near, total)
    for case, exact, want, got, want_greedy, got_greedy in checks:
        assert torch.equal(got[3], want[3]), ("u_out", case)
        for a, b, name in zip(got_greedy, want_greedy,
                              ("seq", "pads", "token", "u_out")):
            assert torch.equal(a, b), ("greedy", name, case)
        assert float(got_greedy[3].max()) == -1.0, ("greedy drew", case)
        for a, b, name in zip(got[:3], want[:3], ("seq", "pads", "token")):
            assert torch.equal(a[exact], b[exact]), (name, case)
        # a near-tie may pick the other candidate, nothing else
        assert bool(((got[2] >= 0) & (got[2] < max(V, 3))).all()), case


@pytest.mark.parametrize("pos", [-1, L - 1, L + 5])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_guard_leaves_memory_unchanged(pos, dtype):
    t = C.make_logits("normal", 3, 320, 25, seed=1).to(dtype)
    st = _state(3, 1)
    seq, pads, token, u = _run(OF.decode_sample, t, pos, st, 25, False,
                               "cuda")
    assert torch.equal(seq, st[1]) and torch.equal(pads, st[3])
    assert torch.equal(token, st[4]) and float(u.max()) == -1.0


def test_without_u_out_and_on_the_current_device_stream():
    t = C.make_logits("normal", 3, 256, 25, seed=1)
    st = _state(3, 1)
    want = _run(R.decode_sample, t, 5, st, 25, False, "cpu")
    seed_t, seq, lens, pads, token = [x.clone().cuda() for x in st]
    OF.decode_sample(t.cuda(), torch.tensor(5).cuda(), seed_t, seq, lens,
                     pads, token, 25, False)
    assert torch.equal(token.cpu(), want[2]) and torch.equal(seq.cpu(), want[0])


# ---- end to end -----------------------------------------------------------

def _model():
    from progen_amd import ProGenBase, ProGenConfig
    cfg = ProGenConfig(num_tokens=256, dim=256, depth=3, heads=4,
                       dim_head=64, window_size=64, seq_len=256,
                       ff_glu=False, global_mlp_depth=1)
    torch.manual_seed(3)
    m = ProGenBase(cfg).to(device="cuda", dtype=torch.bfloat16).eval()
    m.rotary_sin = m.rotary_sin.float()
    m.rotary_cos = m.rotary_cos.float()
    return m


def _primes():
    g = torch.Generator().manual_seed(5)
    return [torch.randint(1, 256, (9,), generator=g),
            torch.randint(1, 256, (5,), generator=g)]


FAST = dict(graph=True, fused=True, fused_linear=True)
LENGTH = 64


def test_greedy_in_graph_sampling_equals_host_sampling():
    from progen_amd.decode import sample_cached_batch
    m = _model()
    want = sample_cached_batch(m, _primes(), LENGTH, **FAST)
    got = sample_cached_batch(m, _primes(), LENGTH, device_sampling=True,
                              **FAST)
    assert torch.equal(got, want), (got, want)


def _host_loop(m, primes, top_k, seed):
    """The graphed step with the logits downloaded and
    ``reference.decode_sample`` applied on the host; also the smallest
    fp64 gap over the live rows of the run."""
    from progen_amd.decode import DecodeCache, GraphedDecodeStep
    B = len(primes)
    seq = torch.zeros(B, LENGTH, dtype=torch.long)
    for i, p in enumerate(primes):
        seq[i, :len(p)] = p
    lens = torch.tensor([len(p) for p in primes])
    pads = (seq[:, 0] == 0).long()
    token = seq[:, 0].clone()
    seed_t = torch.tensor([seed])
    cache = DecodeCache(m, batch=B)
    g = GraphedDecodeStep(m, cache, start_pos=0, fused=True,
                          fused_linear=True)
    min_gap = float("inf")
    for p in range(LENGTH - 1):
        rows = g.step(token).cpu().float()
        live = (pads < 2) & (lens <= p + 1)
        u = R.decode_sample_uniform(seed, p + 1, B, rows.shape[1])
        if bool(live.any()):
            min_gap = min(min_gap, float(C.gap64(rows, u, top_k)[live].min()))
        R.decode_sample(rows, torch.tensor(p), seed_t, seq, lens, pads, token,
                        top_k, False)
    out = seq * (~((seq == 0).long().cumsum(dim=-1) > 1)).long()
    return out, min_gap


def test_stochastic_in_graph_sampling_equals_the_host_loop():
    from progen_amd.decode import sample_cached_batch
    m = _model()
    # chosen by the host loop's own smallest gap, 2.5e-2 for this seed (of
    # seeds 1..16 on an MI355X, 7 and 9 fall under the 1e-3 asserted below)
    seed = 13
    want, min_gap = _host_loop(m, _primes(), 25, seed)
    print(f"MINGAP|seed={seed}|{min_gap:.3e}")
    assert min_gap >= 1e-3, f"choose another seed (smallest gap {min_gap})"
    got = sample_cached_batch(m, _primes(), LENGTH, top_k=25,
                              device_sampling=True, seed=seed, check_every=1,
                              **FAST)
    assert torch.equal(got, want), (got, want)


@pytest.mark.parametrize("graph", [True, False], ids=["graphed", "eager"])
def test_output_does_not_depend_on_check_every(graph):
    from progen_amd.decode import sample_cached_batch
    m = _model()
    kw = dict(FAST, graph=graph)
    outs = [sample_cached_batch(m, _primes(), LENGTH, top_k=25,
                                device_sampling=True, seed=7,
                                check_every=ce, **kw) for ce in (1, 16, 64)]
    assert torch.equal(outs[0], outs[1]), "check_every 16 vs 1"
    assert torch.equal(outs[0], outs[2]), "check_every 64 vs 1"


def test_eager_step_variants_agree_under_device_sampling():
    from progen_amd.decode import sample_cached_batch
    m = _model()
    # forward_step, forward_step_fused and the captured forward_step_static
    for kw in (dict(), dict(fused=True), dict(graph=True)):
        host = sample_cached_batch(m, _primes(), LENGTH, **kw)
        got = sample_cached_batch(m, _primes(), LENGTH, device_sampling=True,
                                  **kw)
        assert torch.equal(got, host), kw


def test_replay_guards_the_position_and_step_is_unchanged():
    from progen_amd.decode import (DecodeCache, DeviceSampler,
                                   GraphedDecodeStep)
    m = _model()
    cache = DecodeCache(m, batch=1)
    seq = torch.zeros(1, 256, dtype=torch.long)
    seq[0, 0] = 4
    s = DeviceSampler(seq, [1], None, None, "cuda")
    g = GraphedDecodeStep(m, cache, start_pos=250, fused=True, sampler=s)
    # the warm-up ran the sampler; the constructor put everything back
    assert torch.equal(s.seq.cpu(), seq) and s.pads.tolist() == [0]
    assert g.token.tolist() == [0]
    with pytest.raises(IndexError):
        g.replay(7)
    assert g.next_pos == 250
    g.replay(2)
    assert g.next_pos == 252 and int(g.pos_dev) == 252
    written = s.seq.cpu()[0, 251:253]
    assert bool(((written >= 0) & (written < 256)).all())
    plain = GraphedDecodeStep(m, DecodeCache(m, batch=1), start_pos=0)
    with pytest.raises(RuntimeError, match="sampler"):
        plain.replay()
