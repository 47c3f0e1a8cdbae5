"""``decode.prefill`` on the CPU (fp32, the reference ops): one forward over a
(B, P) prime leaves the decode cache as P calls of ``forward_step`` do, and
the samplers' ``prefill=True`` emits the tokens of their step loop.

The step-loop side is computed once per batch size, over all 512 positions,
with a snapshot of the cache at every P under test.
"""

import functools

import pytest
import torch

from progen_amd import decode
from progen_amd.config import ProGenConfig
from progen_amd.models.progen import ProGenBase
from progen_amd.ops import functional as OF

SEQ_LEN = 512
PS = [1, 2, 63, 64, 65, 128, 255, 256, 257, 511, 512]
BS = [1, 3]
TOL = dict(rtol=1e-5, atol=1e-5)   # fp32 reassociation only


@functools.lru_cache(maxsize=None)
def _model():
    # tests/test_decode.py's config at seq_len 512, window 64, dim 128: two
    # GLU layers and one SGU layer
    torch.manual_seed(7)
    cfg = ProGenConfig(num_tokens=256, dim=128, depth=3, dim_head=8, heads=2,
                       window_size=64, seq_len=SEQ_LEN, ff_glu=True,
                       global_mlp_depth=1, shift_tokens=True)
    return ProGenBase(cfg).eval()


def _tensors(cache):
    """every tensor of a cache with the dimension its positions run along
    (None: the one-row shift halos)"""
    out = [(f"k{i}", t, 2) for i, t in enumerate(cache.k)]
    out += [(f"v{i}", t, 2) for i, t in enumerate(cache.v)]
    out += [(f"gate_hist{i}", t, 1) for i, t in enumerate(cache.gate_hist)
            if t is not None]
    out += [(f"attn_prev{i}", t, None) for i, t in enumerate(cache.attn_prev)]
    out += [(f"ff_prev{i}", t, None) for i, t in enumerate(cache.ff_prev)]
    return out


def _copy(model, cache):
    new = decode.DecodeCache(model, batch=cache.attn_prev[0].shape[0])
    for (_, dst, _d), (_, src, _s) in zip(_tensors(new), _tensors(cache)):
        dst.copy_(src)
    new.pos = cache.pos
    return new


@functools.lru_cache(maxsize=None)
def _tokens(B):
    g = torch.Generator().manual_seed(100 + B)
    return torch.randint(1, 256, (B, SEQ_LEN), generator=g)


@functools.lru_cache(maxsize=None)
def _stepped(B):
    """{P: (cache after P steps, logits of step P-1)} for every P in PS"""
    model, tok = _model(), _tokens(B)
    cache = decode.DecodeCache(model, batch=B)
    out = {}
    for p in range(SEQ_LEN):
        logits = decode.forward_step(model, tok[:, p], cache)
        if p + 1 in PS:
            out[p + 1] = (_copy(model, cache), logits)
    return out


def _nan_cache(model, B):
    cache = decode.DecodeCache(model, batch=B)
    for _name, t, dim in _tensors(cache):
        if dim is not None:
            t.fill_(float("nan"))
    return cache


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("P", PS)
def test_prefill_leaves_the_cache_of_P_steps(P, B):
    model, tok = _model(), _tokens(B)
    want, want_logits = _stepped(B)[P]
    cache = _nan_cache(model, B)
    untouched = _copy(model, cache)
    logits = decode.prefill(model, tok[:, :P], cache, want_logits=True)

    assert cache.pos == P == want.pos
    for (name, got, dim), (_, ref, _d), (_, nan, _n) in zip(
            _tensors(cache), _tensors(want), _tensors(untouched)):
        if dim is None:
            torch.testing.assert_close(got, ref, **TOL, msg=lambda m: f"{name}: {m}")
            continue
        torch.testing.assert_close(got.narrow(dim, 0, P), ref.narrow(dim, 0, P),
                                   **TOL, msg=lambda m: f"{name}: {m}")
        rest = got.shape[dim] - P
        assert torch.equal(
            got.narrow(dim, P, rest).contiguous().view(torch.int32),
            nan.narrow(dim, P, rest).contiguous().view(torch.int32)), name
    torch.testing.assert_close(logits, want_logits, **TOL)

    if P < SEQ_LEN:
        # the next step reads only rows <= P: the NaN rows must not leak
        nxt = tok[:, P]
        a = decode.forward_step(model, nxt, cache)
        b = decode.forward_step(model, nxt, _copy(model, want))
        torch.testing.assert_close(a, b, **TOL)


def test_prefill_without_logits_returns_none_and_sets_pos_dev():
    model, tok = _model(), _tokens(1)
    cache = decode.DecodeCache(model, batch=1)
    pos_dev = torch.zeros((), dtype=torch.long)
    assert decode.prefill(model, tok[:, :9], cache, pos_dev) is None
    assert cache.pos == 9 and int(pos_dev) == 9


def test_prefill_refuses_a_used_cache_a_long_prime_and_a_bad_shape():
    model, tok = _model(), _tokens(1)
    cache = decode.DecodeCache(model, batch=1)
    decode.forward_step(model, tok[:, 0], cache)
    with pytest.raises(ValueError, match="fresh"):
        decode.prefill(model, tok[:, :4], cache)
    fresh = decode.DecodeCache(model, batch=1)
    with pytest.raises(IndexError, match="seq_len"):
        decode.prefill(model, torch.ones(1, SEQ_LEN + 1, dtype=torch.long),
                       fresh)
    with pytest.raises(ValueError, match="tokens"):
        decode.prefill(model, tok[0, :4], fresh)
    with pytest.raises(ValueError, match="tokens"):
        decode.prefill(model, _tokens(3)[:, :4], fresh)
    assert fresh.pos == 0


def test_prefill_supported_on_the_cpu():
    model = _model()
    assert all(decode.prefill_supported(model, P, "cpu") for P in PS)
    assert not decode.prefill_supported(model, 0, "cpu")
    assert not decode.prefill_supported(model, SEQ_LEN + 1, "cpu")
    assert decode.PREFILL_MIN_TOKENS >= 2


# ---------------------------------------------------------------------------
# the samplers
# ---------------------------------------------------------------------------

LENGTH = 96
RAGGED = (5, 9, 70)


def _primes(lens):
    g = torch.Generator().manual_seed(5)
    return [torch.randint(1, 256, (n,), generator=g) for n in lens]


def test_sample_cached_prefill_emits_the_same_tokens():
    model = _model()
    prime = _primes((70,))[0]
    # the host sampler of one row always adds gumbel noise: the same seeded
    # stream in both runs, one draw per sampled token
    def gen():
        return torch.Generator().manual_seed(11)

    want = decode.sample_cached(model, prime, LENGTH, add_bos=True,
                                generator=gen())
    got = decode.sample_cached(model, prime, LENGTH, add_bos=True,
                               generator=gen(), prefill=True)
    assert torch.equal(got, want)
    assert (got[71:] != 0).any()  # something was sampled


@pytest.mark.parametrize("device_sampling", [False, True])
def test_sample_cached_batch_prefill_emits_the_same_tokens(device_sampling):
    model = _model()
    kw = dict(device_sampling=device_sampling)
    want = decode.sample_cached_batch(model, _primes(RAGGED), LENGTH, **kw)
    got = decode.sample_cached_batch(model, _primes(RAGGED), LENGTH,
                                     prefill=True, **kw)
    assert torch.equal(got, want)
    if device_sampling:  # and the single-row entry point
        one = decode.sample_cached(model, _primes(RAGGED)[2], LENGTH,
                                   device_sampling=True, prefill=True)
        assert torch.equal(one, want[2])


def test_prefill_goes_through_the_prefill_ops(monkeypatch):
    model = _model()
    calls = {"attn": 0, "sgu": 0}
    real_attn, real_sgu = OF.prefill_attention, OF.prefill_sgu

    def attn(*a, **k):
        calls["attn"] += 1
        return real_attn(*a, **k)

    def sgu(*a, **k):
        calls["sgu"] += 1
        return real_sgu(*a, **k)

    monkeypatch.setattr(OF, "prefill_attention", attn)
    monkeypatch.setattr(OF, "prefill_sgu", sgu)
    prime = _primes((70,))[0]
    decode.sample_cached(model, prime, 80)
    decode.sample_cached_batch(model, _primes(RAGGED), 80)
    assert calls == {"attn": 0, "sgu": 0}
    decode.sample_cached(model, prime, 80, prefill=True)
    assert calls == {"attn": 3, "sgu": 1}   # once per layer, one SGU layer
    decode.sample_cached_batch(model, _primes(RAGGED), 80, prefill=True)
    decode.sample_cached_batch(model, _primes(RAGGED), 80, prefill=True,
                               device_sampling=True)
    assert calls == {"attn": 9, "sgu": 3}


def test_unsupported_prefill_keeps_the_step_loop(monkeypatch):
    model = _model()
    prime = _primes((70,))[0]
    def gen():
        return torch.Generator().manual_seed(11)

    want = decode.sample_cached(model, prime, 80, generator=gen())
    want_b = decode.sample_cached_batch(model, _primes(RAGGED), 80)

    def boom(*a, **k):
        raise AssertionError("prefill must not run")

    monkeypatch.setattr(decode, "prefill", boom)
    monkeypatch.setattr(decode, "prefill_supported", lambda *a: False)
    assert torch.equal(decode.sample_cached(model, prime, 80, prefill=True,
                                            generator=gen()), want)
    for ds in (False, True):
        got = decode.sample_cached_batch(model, _primes(RAGGED), 80,
                                         prefill=True, device_sampling=ds)
        assert torch.equal(got, want_b)
    # a prefix too short to prefill (a one-token prime) never asks
    monkeypatch.setattr(decode, "prefill_supported", boom)
    decode.sample_cached_batch(model, [prime[:1], prime], 74, prefill=True)


def test_device_sampler_counts_the_pads_of_what_is_written():
    seq = torch.tensor([[5, 0, 6, 0, 0, 0], [0, 1, 2, 3, 0, 0]])
    assert decode.DeviceSampler(seq, [3, 4], None, None, "cpu").pads.tolist() \
        == [0, 1]
    s = decode.DeviceSampler(seq, [3, 4], None, None, "cpu", written=3)
    assert s.pads.tolist() == [1, 1] and s.pads.dtype == torch.long


@pytest.mark.parametrize("device_sampling", [False, True])
def test_a_pad_inside_the_common_prefix_is_counted(monkeypatch,
                                                   device_sampling):
    """A model that always emits 0: each row ends at its first sampled
    token if its prime holds one pad already. Row 0's only pad is at
    column 1, inside the prefilled prefix; were it not counted, the batch
    would run one step longer."""
    torch.manual_seed(7)
    model = ProGenBase(_model().cfg).eval()
    with torch.no_grad():
        model.to_logits.bias[0] = 1e4
    primes = [torch.tensor([5, 0, 6, 7, 8, 9, 10, 11, 12]),
              torch.tensor([0, 1, 2, 3, 4, 5])]
    steps = []
    real = decode.forward_step
    monkeypatch.setattr(decode, "forward_step",
                        lambda *a, **k: steps.append(1) or real(*a, **k))
    kw = dict(device_sampling=device_sampling, check_every=1)
    want = decode.sample_cached_batch(model, primes, 40, **kw)
    assert len(steps) == 9      # positions 0..8; row 0 ends at column 9
    del steps[:]
    got = decode.sample_cached_batch(model, primes, 40, prefill=True, **kw)
    assert len(steps) == 4      # positions 5..8 after a 5-token prefill
    assert torch.equal(got, want)
    assert got[0].tolist()[:10] == [5, 0, 6, 7, 8, 9, 10, 11, 12, 0]
    assert got[1].tolist()[:7] == [0, 1, 2, 3, 4, 5, 0]
