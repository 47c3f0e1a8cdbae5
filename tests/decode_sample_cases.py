"""Inputs and oracles shared by tests/test_decode_sample.py (CPU) and
tests/test_gpu_decode_sample.py (GPU): the logit families on which the
sampler's quirks show, the host sampler written from
``reference.select_top_k`` + ``gumbel_noise``'s formula, and the fp64 gap
that names a near-tie.

Every logit is a bf16 value with |t| <= 40, so the bf16 and the fp32 kernel
see the same row."""

import torch

from progen_amd.ops import reference as R

FAMILIES = ("normal", "ties", "negative")


def make_logits(family: str, B: int, V: int, k: int, seed: int) -> torch.Tensor:
    """(B, V) fp32 logits holding bf16 values.

    normal:   N(0, 3^2), clamped to |t| <= 40.
    ties:     normal, then the largest value of each row copied over its
              third-smallest entry and the k-th largest value (the top-k
              threshold) over its two smallest: ties above the threshold
              and AT it.
    negative: -40 + |N(0, 2^2)| clamped to [-40, -30]: every selected score
              t + g is negative (g < 17), so an excluded entry (score 0)
              must win."""
    g = torch.Generator().manual_seed(1000 * seed + V + 7 * k + 13 * B)
    t = torch.randn(B, V, generator=g) * 3.0
    if family == "negative":
        t = (-40.0 + (t * (2.0 / 3.0)).abs()).clamp(-40.0, -30.0)
    t = t.clamp(-40.0, 40.0).bfloat16().float()
    if family == "ties" and V >= 4:
        kk = min(max(k, 1), V)
        for b in range(B):
            order = t[b].argsort(descending=True)
            t[b, order[-3]] = t[b, order[0]]
            vals, order = t[b].sort(descending=True)
            t[b, order[-1]] = vals[kk - 1]
            t[b, order[-2]] = vals[kk - 1]
    return t


def host_scores(t: torch.Tensor, u: torch.Tensor, k: int, greedy: bool = False,
                mutant: str = None) -> torch.Tensor:
    """The scores ``decode.sample_cached_batch`` argmaxes on the host, from
    the uniforms ``u``: ``select_top_k`` + the gumbel formula, fp32.
    ``mutant`` breaks one quirk on purpose (None: the real thing)."""
    t = t.float()
    if greedy:
        return t
    eps = 1e-20
    noise = -torch.log(-torch.log(u + eps) + eps)
    if k <= 0:
        return t + noise
    if mutant == "kth_included":
        values, _ = t.topk(k, dim=-1)
        mask = t >= values.amin(dim=-1, keepdim=True)
        rows = torch.where(mask, t, torch.zeros_like(t))
    else:
        mask, rows = R.select_top_k(t, k)
    if mutant == "excluded_neg_inf":
        rows = torch.where(mask, t, torch.full_like(t, float("-inf")))
    if mutant != "noise_unmasked":
        noise = noise * mask
    return rows + noise


def first_argmax(scores: torch.Tensor, mutant: str = None) -> torch.Tensor:
    if mutant == "ties_to_last":
        V = scores.shape[-1]
        return V - 1 - scores.flip(-1).argmax(dim=-1)
    return scores.argmax(dim=-1)


def gap64(t: torch.Tensor, u: torch.Tensor, k: int) -> torch.Tensor:
    """Per row, in fp64: the best score minus the largest score strictly
    below it (inf when every score is equal). Under 1e-4 is a near-tie: the
    kernel's fp32 logs may order the two differently."""
    t = t.double()
    eps = 1e-20
    g = -torch.log(-torch.log(u.double() + eps) + eps)
    if k > 0:
        sel = (t.unsqueeze(1) >= t.unsqueeze(2)).sum(dim=-1) < k
        s = torch.where(sel, t + g, torch.zeros_like(t))
    else:
        s = t + g
    best = s.amax(dim=-1, keepdim=True)
    below = torch.where(s < best, s, torch.full_like(s, float("-inf")))
    return (best - below.amax(dim=-1, keepdim=True)).squeeze(-1)


def state(B: int, L: int, lens=None, seed: int = 0, device="cpu"):
    """Fresh sampler state: seq of 7s (so a write shows and no pad is
    counted by accident), lens (default 0: nothing primed), pads 0, token
    -1, and the (1,) seed."""
    seq = torch.full((B, L), 7, dtype=torch.long)
    lens = torch.zeros(B, dtype=torch.long) if lens is None \
        else torch.as_tensor(lens, dtype=torch.long)
    pads = torch.zeros(B, dtype=torch.long)
    token = torch.full((B,), -1, dtype=torch.long)
    seed_t = torch.tensor([seed], dtype=torch.long)
    return [x.to(device) for x in (seed_t, seq, lens, pads, token)]
