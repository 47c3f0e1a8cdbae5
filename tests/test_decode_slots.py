"""The slot twins of the decode-step references (ops/reference.py,
``*_slots``) and ``decode.forward_step_slots`` on the CPU.

A slot op gives every batch row its own position: row b must compute what
the scalar reference computes for that row alone at pos[b], a row at
position 0 must not see the slot's old ``prev`` row, and an idle row
(pos[b] < 0) must change nothing and come back as zeros. Stepping every row
from 0 with stream = row index is then ``sample_cached_batch`` with the
device sampler, token for token."""

import pytest
import torch

from progen_amd import ProGenBase, ProGenConfig
from progen_amd.decode import (DecodeCache, forward_step_slots,
                               sample_cached_batch)
from progen_amd.ops import functional as OF
from progen_amd.ops import reference as R

POS = [0, 3, -1, 9, 15]
B = len(POS)


def _pos():
    return torch.tensor(POS, dtype=torch.long)


def _live():
    return [b for b, p in enumerate(POS) if p >= 0]


def test_ln_shift_rows_equal_the_scalar_reference_and_pos0_ignores_prev():
    torch.manual_seed(0)
    D = 32
    h, res, prev = torch.randn(B, D), torch.randn(B, D), torch.randn(B, D)
    g = torch.randn(D)
    for shift in (True, False):
        for use_res in (True, False):
            h1, p1 = h.clone(), prev.clone()
            y = R.decode_ln_shift_slots(h1, res if use_res else None, g, p1,
                                        _pos(), shift)
            for b in _live():
                h2 = h[b:b + 1].clone()
                p2 = prev[b:b + 1].clone()
                if POS[b] == 0:
                    p2.zero_()
                want = R.decode_ln_shift(h2, res[b:b + 1] if use_res else None,
                                         g, p2, shift)
                assert torch.equal(y[b:b + 1], want)
                assert torch.equal(h1[b:b + 1], h2)
                assert torch.equal(p1[b:b + 1], p2)
            # the idle row
            assert torch.equal(y[2], torch.zeros(D))
            assert torch.equal(h1[2], h[2]) and torch.equal(p1[2], prev[2])
    # position 0 with a poisoned prev row: nothing of it reaches y
    p1 = prev.clone()
    p1[0] = float("nan")
    y = R.decode_ln_shift_slots(h.clone(), None, g, p1, _pos(), True)
    assert torch.isfinite(y).all() and torch.equal(y[0, :D // 2],
                                                   torch.zeros(D // 2))


def test_attention_rows_equal_the_scalar_reference():
    torch.manual_seed(1)
    H, N, dh, window = 2, 16, 8, 8
    sin, cos = R.fixed_pos_embedding(N, dh)
    qkv = torch.randn(B, 3 * H * dh)
    k, v = torch.randn(B, H, N, dh), torch.randn(B, H, N, dh)
    k1, v1 = k.clone(), v.clone()
    out = R.decode_attention_slots(qkv, sin, cos, _pos(), k1, v1, window)
    for b in _live():
        k2, v2 = k[b:b + 1].clone(), v[b:b + 1].clone()
        want = R.decode_attention(qkv[b:b + 1], sin, cos,
                                  torch.tensor(POS[b]), k2, v2, window)
        assert torch.equal(out[b:b + 1], want)
        assert torch.equal(k1[b:b + 1], k2) and torch.equal(v1[b:b + 1], v2)
    assert torch.equal(out[2], torch.zeros(H * dh))
    assert torch.equal(k1[2], k[2]) and torch.equal(v1[2], v[2])


def test_sgu_rows_equal_the_scalar_reference():
    torch.manual_seed(2)
    N, d2 = 16, 8
    h, g = torch.randn(B, 2 * d2), torch.randn(d2)
    hist = torch.randn(B, N, d2)
    w, bias = torch.randn(N, N), torch.randn(N, 1)
    h1 = hist.clone()
    out = R.decode_sgu_slots(h, g, h1, w, bias, _pos())
    for b in _live():
        h2 = hist[b:b + 1].clone()
        want = R.decode_sgu(h[b:b + 1], g, h2, w, bias, torch.tensor(POS[b]))
        assert torch.equal(out[b:b + 1], want)
        assert torch.equal(h1[b:b + 1], h2)
    assert torch.equal(out[2], torch.zeros(d2))
    assert torch.equal(h1[2], hist[2])


def test_sample_rows_equal_the_scalar_reference():
    """Uniform controls with stream = row index at one position are
    ``decode_sample``; the positions advance; an idle row is untouched."""
    torch.manual_seed(3)
    V, L, p = 40, 16, 4
    logits = torch.randn(B, V) * 3
    for top_k, seed in ((0, -1), (5, 77), (0, 9)):
        seq = torch.randint(1, V, (B, L))
        lens = torch.tensor([2, 9, 1, 1, 6])
        pads, token = torch.zeros(B, dtype=torch.long), torch.zeros(
            B, dtype=torch.long)
        s0, p0, t0, u0 = seq.clone(), pads.clone(), token.clone(), \
            torch.zeros(B, V)
        R.decode_sample(logits, torch.tensor(p), torch.tensor([max(seed, 0)]),
                        s0, lens, p0, t0, top_k, seed < 0, u0)
        pos = torch.tensor([p, p, -1, p, p])
        ctl = torch.stack([lens, torch.full((B,), L), torch.full((B,), top_k),
                           torch.full((B,), seed), torch.arange(B)], dim=1)
        s1, p1, t1, u1 = seq.clone(), pads.clone(), token.clone(), \
            torch.zeros(B, V)
        OF.decode_sample_slots(logits, pos, t1, s1, p1, ctl, u1)
        live = [0, 1, 3, 4]
        assert torch.equal(s1[live], s0[live])
        assert torch.equal(p1[live], p0[live])
        assert torch.equal(t1[live], t0[live])
        assert torch.equal(u1[live], u0[live])
        assert pos.tolist() == [p + 1, p + 1, -1, p + 1, p + 1]
        assert torch.equal(s1[2], seq[2]) and int(p1[2]) == 0 \
            and int(t1[2]) == 0 and not u1[2].any()


def test_sample_retires_rows_and_keeps_streams_apart():
    V, L = 12, 8
    logits = torch.zeros(4, V)
    logits[:, 0] = 5.0                      # greedy rows sample a pad
    seq = torch.zeros(4, L, dtype=torch.long)
    pads = torch.tensor([1, 0, 0, 0])
    token = torch.full((4,), 7)
    pos = torch.tensor([2, 2, 3, 6])
    #            len limit top_k seed stream
    ctl = torch.tensor([[0, 8, 0, -1, 0],    # second pad: retires
                        [0, 8, 0, -1, 0],    # first pad: goes on
                        [0, 5, 0, -1, 0],    # writes limit - 1: retires
                        [0, 7, 0, -1, 0]])   # w >= limit on entry: retires,
    seq[3, 7] = 9                            # and nothing else changes
    OF.decode_sample_slots(logits, pos, token, seq, pads, ctl)
    assert pos.tolist() == [-1, 3, -1, -1]
    assert pads.tolist() == [2, 1, 1, 0]
    assert token.tolist() == [0, 0, 0, 7]
    assert int(seq[3, 7]) == 9
    # a request's draws depend on its stream, not on the slot it landed in
    torch.manual_seed(4)
    logits = torch.randn(3, V)
    logits[2] = logits[0]
    u = torch.zeros(3, V)
    ctl = torch.tensor([[0, 8, 0, 5, 1], [0, 8, 0, 5, 0], [0, 8, 0, 5, 1]])
    token = torch.zeros(3, dtype=torch.long)
    OF.decode_sample_slots(logits, torch.tensor([1, 1, 1]), token,
                           torch.zeros(3, L, dtype=torch.long),
                           torch.zeros(3, dtype=torch.long), ctl, u)
    assert torch.equal(u[0], u[2]) and not torch.equal(u[0], u[1])
    assert int(token[0]) == int(token[2])
    assert torch.equal(u[0], R.decode_sample_uniform(5, 2, 2, V)[1])


def _tiny():
    cfg = ProGenConfig(num_tokens=256, dim=16, depth=2, dim_head=8, heads=2,
                       window_size=8, seq_len=64, global_mlp_depth=1)
    torch.manual_seed(5)
    return ProGenBase(cfg).eval(), cfg


PRIMES = [[0, 35, 32, 77], [0, 35, 32, 71, 65], [0, 40], [0, 35, 32, 77, 75,
                                                         86, 76]]


@pytest.mark.parametrize("top_k,seed", [(None, None), (25, 123)])
@pytest.mark.parametrize("fused_linear", [False, True])
def test_slot_step_loop_equals_sample_cached_batch(top_k, seed, fused_linear):
    model, cfg = _tiny()
    length = 48
    primes = [torch.tensor(p) for p in PRIMES]
    want = sample_cached_batch(model, primes, length, top_k=top_k, seed=seed,
                               fused=True, fused_linear=fused_linear,
                               device_sampling=True)
    n = len(primes)
    cache = DecodeCache(model, batch=n)
    seq = torch.zeros(n, cfg.seq_len, dtype=torch.long)
    for i, p in enumerate(primes):
        seq[i, :len(p)] = p
    token = seq[:, 0].clone()
    pads = (token == 0).long()
    pos = torch.zeros(n, dtype=torch.long)
    ctl = torch.tensor([[len(p), length, top_k or 0,
                         -1 if seed is None else seed, i]
                        for i, p in enumerate(primes)])
    steps = 0
    while (pos >= 0).any():
        logits = forward_step_slots(model, token, cache, pos,
                                    fused_linear=fused_linear)
        OF.decode_sample_slots(logits, pos, token, seq, pads, ctl)
        steps += 1
        assert steps < length
    out = seq[:, :length]
    out = out * (~((out == 0).long().cumsum(dim=-1) > 1)).long()
    assert torch.equal(out, want)


def test_an_idle_row_leaves_the_step_state_alone():
    model, cfg = _tiny()
    cache = DecodeCache(model, batch=2)
    for t in cache.k + cache.v + cache.attn_prev + cache.ff_prev + \
            [g for g in cache.gate_hist if g is not None]:
        t[1].fill_(float("nan"))   # whatever an old request left behind
    pos = torch.tensor([0, -1])
    token = torch.tensor([0, 3])
    logits = forward_step_slots(model, token, cache, pos)
    assert torch.isfinite(logits).all()
    for t in cache.k + cache.v + cache.attn_prev + cache.ff_prev + \
            [g for g in cache.gate_hist if g is not None]:
        assert torch.isnan(t[1]).all()
    # and row 0 is what it computes alone
    alone = DecodeCache(model, batch=1)
    want = forward_step_slots(model, token[:1], alone, pos[:1])
    # (another batch size may reduce in another order)
    torch.testing.assert_close(logits[:1], want, rtol=1e-5, atol=1e-6)
