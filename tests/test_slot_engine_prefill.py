"""``SlotEngine(prefill=True)`` on the CPU (fp32, the reference ops), on the
model of tests/test_decode_prefill.py: a request whose prime is prefilled at
admission returns exactly the tokens of the engine that teacher-forces it,
the routing sends the right primes each way, ``reference.prefill_attention``
and ``reference.prefill_sgu`` place their rows as ``admit`` says, and
serve.py exposes the flag.
"""

import functools

import pytest
import torch

from progen_amd import decode
from progen_amd.config import ProGenConfig
from progen_amd.engine import PREFILL_MIN_TOKENS, SlotEngine
from progen_amd.models.progen import ProGenBase
from progen_amd.ops import functional as OF
from progen_amd.ops import reference as R

SEQ_LEN = 512


@functools.lru_cache(maxsize=None)
def _model():
    torch.manual_seed(7)
    cfg = ProGenConfig(num_tokens=256, dim=128, depth=3, dim_head=8, heads=2,
                       window_size=64, seq_len=SEQ_LEN, ff_glu=True,
                       global_mlp_depth=1, shift_tokens=True)
    return ProGenBase(cfg).eval()


def _prime(n, seed=0, pads=()):
    g = torch.Generator().manual_seed(1000 + 7 * n + seed)
    p = torch.randint(1, 256, (n,), generator=g)
    for i in pads:
        p[i] = 0
    return p


@pytest.fixture
def forwards(monkeypatch):
    """Counts of (prefill forwards' attention calls, their batch rows)."""
    calls = []
    real = OF.prefill_attention

    def counted(qkv, *a, **k):
        calls.append(qkv.shape[0])
        return real(qkv, *a, **k)

    monkeypatch.setattr(OF, "prefill_attention", counted)
    return calls


def _both(requests, slots, forwards, **kw):
    """Serve (prime, length, sampling) requests, all queued at once, through
    the engine without and with prefill; returns (plain results, prefilled
    results, the prefilling engine)."""
    out = []
    for prefill in (False, True):
        e = SlotEngine(_model(), slots, prefill=prefill,
                       **(kw if prefill else {}))
        tickets = [e.submit([p], n, **s) for p, n, s in requests]
        e.run_until_idle()
        out.append([t.wait() for t in tickets])
        if not prefill:
            assert not forwards, "prefill ran without the flag"
    return out[0], out[1], e


def _layers():
    return len(_model().layers)


def test_one_ragged_request(forwards):
    primes = [_prime(n) for n in (20, 3, 70, 9, 130)]
    a = SlotEngine(_model(), 5).generate(primes, 160)
    assert not forwards
    e = SlotEngine(_model(), 5, prefill=True, prefill_min_tokens=8)
    b = e.generate(primes, 160)
    assert torch.equal(a, b)
    # 19 and 8 positions share the 64-row bucket but prefill_rows is 1;
    # 69 and 129 take the 128- and 192-row ones; 2 positions are stepped
    assert e.prefills == 4 and len(forwards) == 4 * _layers()
    assert e.prefilled_positions == 19 + 69 + 8 + 129


def test_staggered_requests_reuse_a_slot_that_holds_the_previous_one(forwards):
    # 2 slots, 4 requests: the third and fourth land in slots whose caches
    # still hold longer, finished requests; one of them is prefilled over
    # those rows and one is stepped
    reqs = [(_prime(100), 140, {}), (_prime(40), 90, {}),
            (_prime(30, 1), 80, {}), (_prime(5), 60, {})]
    a, b, e = _both(reqs, 2, forwards, prefill_min_tokens=8)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert e.prefills == 3 and e.steps > 0


@pytest.mark.parametrize("pads,prefilled", [((0,), 1), ((5,), 1),
                                            ((0, 11), 0), ((3, 4), 0)],
                         ids=["bos", "one-inside", "bos+one", "two-inside"])
def test_primes_with_pads(forwards, pads, prefilled):
    # one pad (a BOS, or one inside) is prefilled and counted at admission;
    # two retire the request inside its prime: not prefilled
    reqs = [(_prime(24, pads=pads), 60, {})]
    a, b, e = _both(reqs, 1, forwards, prefill_min_tokens=8)
    assert torch.equal(a[0], b[0])
    assert e.prefills == prefilled
    if len(pads) == 2:
        assert not b[0][0, pads[1] + 1:].any(), "zeroed after the second pad"


def test_primes_below_and_at_prefill_min_tokens(forwards):
    # min 16 positions: a 16-token prime has 15 (stepped), a 17-token one 16
    for n, want in ((16, 0), (17, 1)):
        a, b, e = _both([(_prime(n), 50, {})], 1, forwards,
                        prefill_min_tokens=16)
        assert torch.equal(a[0], b[0])
        assert e.prefills == want, n
        del forwards[:]
    assert SlotEngine(_model(), 1, prefill=True).prefill_min_tokens == \
        PREFILL_MIN_TOKENS


@pytest.mark.parametrize("rows", [1, 2])
def test_more_admissions_than_prefill_rows(forwards, rows):
    # 5 slots admit in one cycle: three primes of the 64-row bucket, one of
    # the 128-row one, one stepped
    reqs = [(_prime(n, i), 150, {})
            for i, n in enumerate((20, 33, 64, 100, 4))]
    a, b, e = _both(reqs, 5, forwards, prefill_rows=rows,
                    prefill_min_tokens=8)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert e.prefills == (4 if rows == 1 else 3)
    assert sorted(set(forwards)) == [rows]
    assert len(forwards) == e.prefills * _layers()


@pytest.mark.parametrize("sampling", [dict(), dict(top_k=25, seed=11)],
                         ids=["greedy", "top_k-seed"])
def test_greedy_and_seeded_sampling(forwards, sampling):
    reqs = [(_prime(50), 120, sampling), (_prime(12, 2), 70, sampling),
            (_prime(70, 3), 100, sampling)]
    a, b, e = _both(reqs, 2, forwards, prefill_min_tokens=8)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert e.prefills == 3


def test_the_engine_equals_sample_cached_batch_with_prefill(forwards):
    p = _prime(40)
    want = decode.sample_cached_batch(_model(), [p], 90, prefill=True)
    n = len(forwards)
    assert n, "the sampler prefilled"
    got = SlotEngine(_model(), 1, prefill=True).generate([p], 90)
    assert len(forwards) == 2 * n
    assert torch.equal(got, want)


def test_bad_arguments():
    with pytest.raises(ValueError, match="prefill_rows"):
        SlotEngine(_model(), 1, prefill=True, prefill_rows=0)
    with pytest.raises(ValueError, match="prefill_min_tokens"):
        SlotEngine(_model(), 1, prefill=True, prefill_min_tokens=0)


# ---- the reference ops with admit -------------------------------------------

NAN = float("nan")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _admit(*rows):
    return torch.tensor(rows, dtype=torch.long)


def _check_rows(got, nan, want, slot, rows, dim):
    """``got``: rows < ``rows`` of cache row ``slot`` are ``want``'s (the
    no-admit result's batch row), everything else keeps ``nan``'s bits."""
    expect = nan.clone()
    if slot is not None:
        expect[slot].narrow(dim - 1, 0, rows).copy_(
            want.narrow(dim - 1, 0, rows))
    assert torch.equal(_bits(got), _bits(expect))


@pytest.mark.parametrize("rows", [1, 63, 64])
def test_reference_prefill_attention_with_admit(rows):
    B, H, N, Nc, S, dh = 2, 2, 64, 128, 3, 8
    g = torch.Generator().manual_seed(rows)
    qkv = torch.randn(B, N, 3 * H * dh, generator=g)
    sin, cos = R.fixed_pos_embedding(Nc, dh)
    k0, v0 = torch.zeros(B, H, Nc, dh), torch.zeros(B, H, Nc, dh)
    out0 = R.prefill_attention(qkv, sin, cos, H, 64, k0, v0, N)

    nan = torch.full((S, H, Nc, dh), NAN)
    # batch row 0 -> slot 2; batch row 1 names no slot, then slot S
    for second in ([-1, N], [S, N]):
        k, v = nan.clone(), nan.clone()
        out = R.prefill_attention(qkv, sin, cos, H, 64, k, v, N,
                                  admit=_admit([2, rows], second))
        assert torch.equal(out, out0)
        _check_rows(k, nan, k0[0], 2, rows, 2)
        _check_rows(v, nan, v0[0], 2, rows, 2)
    # rows <= 0 stores nothing; rows past P stop at P
    k, v = nan.clone(), nan.clone()
    R.prefill_attention(qkv, sin, cos, H, 64, k, v, 10,
                        admit=_admit([0, 0], [1, 500]))
    _check_rows(k, nan, k0[1], 1, 10, 2)
    _check_rows(v, nan, v0[1], 1, 10, 2)


@pytest.mark.parametrize("rows", [1, 63, 64])
def test_reference_prefill_sgu_with_admit(rows):
    B, N, Nc, S, d2 = 2, 64, 128, 3, 16
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(B, N, 2 * d2, generator=g)
    gw = torch.randn(d2, generator=g)
    w = torch.randn(Nc, Nc, generator=g) * 0.05
    bias = torch.randn(Nc, 1, generator=g)
    h0 = torch.zeros(B, Nc, d2)
    out0 = R.prefill_sgu(x, gw, w, bias, h0, N)

    nan = torch.full((S, Nc, d2), NAN)
    for second in ([-1, N], [S, N]):
        h = nan.clone()
        out = R.prefill_sgu(x, gw, w, bias, h, N,
                            admit=_admit([2, rows], second))
        assert torch.equal(out, out0)
        _check_rows(h, nan, h0[0], 2, rows, 1)
    h = nan.clone()
    R.prefill_sgu(x, gw, w, bias, h, 10, admit=_admit([0, -3], [1, 500]))
    _check_rows(h, nan, h0[1], 1, 10, 1)


def test_functional_ops_pass_admit_through():
    B, H, N, Nc, dh = 1, 2, 64, 64, 8
    qkv = torch.randn(B, N, 3 * H * dh)
    sin, cos = R.fixed_pos_embedding(Nc, dh)
    k = torch.full((2, H, Nc, dh), NAN)
    v = k.clone()
    OF.prefill_attention(qkv, sin, cos, H, 64, k, v, N, admit=_admit([1, 5]))
    assert torch.isfinite(k[1, :, :5]).all() and k[0].isnan().all()
    assert k[1, :, 5:].isnan().all() and torch.isfinite(v[1, :, :5]).all()
    x = torch.randn(B, N, 32)
    h = torch.full((2, Nc, 16), NAN)
    OF.prefill_sgu(x, torch.ones(16), torch.randn(Nc, Nc), torch.zeros(Nc, 1),
                   h, N, admit=_admit([1, 5]))
    assert torch.isfinite(h[1, :5]).all() and h[0].isnan().all()
    assert h[1, 5:].isnan().all()


def test_prefill_rows_fills_the_rows_prefill_fills():
    # the capturable loop against ``prefill`` on a 1-row cache: same ops on
    # the same shapes, so the same bits; the other slot keeps its NaNs
    m = _model()
    p = _prime(70)
    one = decode.DecodeCache(m, batch=1)
    decode.prefill(m, p[None], one)
    two = decode.DecodeCache(m, batch=2)
    tensors = two.k + two.v + two.gate_hist + two.attn_prev + two.ff_prev
    for t in tensors:
        if t is not None:
            t.fill_(NAN)
    tokens = torch.zeros(1, 128, dtype=torch.long)
    tokens[0, :70] = p
    decode.prefill_rows(m, tokens, two, _admit([1, 70]),
                        torch.tensor([0, 69]), torch.tensor([-1, 0]))
    for name in ("k", "v", "gate_hist", "attn_prev", "ff_prev"):
        for got, want in zip(getattr(two, name), getattr(one, name)):
            if got is None:
                continue
            assert got[0].isnan().all(), name
            if name.endswith("prev"):
                assert torch.equal(got[1], want[0]), name
                continue
            dim = 1 if name != "gate_hist" else 0
            assert torch.equal(got[1].narrow(dim, 0, 70),
                               want[0].narrow(dim, 0, 70)), name
            assert got[1].narrow(dim, 70, SEQ_LEN - 70).isnan().all(), name


# ---- serve.py -----------------------------------------------------------------

def _client(**kw):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from serve import create_app
    cfg = ProGenConfig(num_tokens=256, dim=16, depth=2, dim_head=8, heads=2,
                       window_size=8, seq_len=64, global_mlp_depth=1)
    torch.manual_seed(5)
    module = ProGenBase(cfg).eval()
    return TestClient(create_app(module, cfg, **kw))


ON = dict(fused=True, device_sampling=True)


def test_serve_info_and_generate_through_slot_prefill(forwards):
    assert _client().get("/info").json()["slot_prefill"] is False
    # BOS + 14 bytes: 14 positions to prefill, one pad
    body = {"primes": ["# MKTAYIAKQRQI", "# GA"], "num_tokens": 48,
            "top_k": 0}
    with _client(slots=2, **ON) as off:
        assert off.get("/info").json()["slot_prefill"] is False
        want = off.post("/generate", json=body).json()
    assert not forwards
    with _client(slots=2, slot_prefill=True, **ON) as on:
        info = on.get("/info").json()
        assert info["slot_prefill"] is True and info["slots"] == 2
        got = on.post("/generate", json=body).json()
    assert forwards, "the long prime was prefilled"
    assert got["tokens"] == want["tokens"]
    assert got["sequences"] == want["sequences"]


def test_serve_usage_errors():
    import serve
    from click.testing import CliRunner
    with pytest.raises(ValueError, match="slot_prefill needs slots"):
        _client(slot_prefill=True, **ON)
    with pytest.raises(ValueError, match="slots needs"):
        _client(slots=2, slot_prefill=True)
    # --slots with --prefill stays refused, with its message
    with pytest.raises(ValueError, match="slots cannot be combined with "
                                         "prefill"):
        _client(slots=2, prefill=True, slot_prefill=True, **ON)
    for argv, what in (
            (["--slot-prefill"], "--slot-prefill needs --slots"),
            (["--slots", "2", "--slot-prefill"], "--slots needs"),
            (["--slots", "2", "--fused", "--device-sampling", "--prefill",
              "--slot-prefill"], "--slots cannot be combined with --prefill")):
        r = CliRunner().invoke(serve.main, argv)
        assert r.exit_code == 2, r.output
        assert "Usage:" in r.output and what in r.output
