"""The decode linear op above the kernel, on the CPU: the reference, the
routing predicate, the ``fused_linear`` switch of the decode step and
samplers (where it must not change a bit), and the CLI / serve plumbing."""

import pytest
import torch
import torch.nn.functional as F

from progen_amd import decode
from progen_amd.config import ProGenConfig
from progen_amd.models.progen import ProGenBase
from progen_amd.ops import functional as OF, reference as R

BF, F32 = torch.bfloat16, torch.float32


# ---------------------------------------------------------------------------
# reference and functional
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("with_bias", [True, False])
def test_reference_equals_the_separate_ops(dtype, with_bias):
    torch.manual_seed(0)
    x = torch.randn(3, 64).to(dtype)
    w = torch.randn(32, 64).to(dtype)
    b = torch.randn(32).to(dtype) if with_bias else None
    h = F.linear(x, w, b)
    for fn in (R.decode_linear, OF.decode_linear):
        assert torch.equal(fn(x, w, b, "none"), h)
        assert torch.equal(fn(x, w, b, "gelu"), R.gelu(h))
        assert torch.equal(fn(x, w, b, "glu"), R.glu_gelu(h))
        assert fn(x, w, b, "glu").shape == (3, 16)
        with pytest.raises(ValueError):
            fn(x, w, b, "relu")


def test_glu_pairs_column_j_with_column_j_plus_half():
    x = torch.eye(4)
    w = torch.arange(32.0).reshape(8, 4) / 8
    b = torch.arange(8.0) / 4
    got = R.decode_linear(x, w, b, "glu")
    h = x @ w.t() + b
    want = h[:, :4] * F.gelu(h[:, 4:], approximate="tanh")
    assert torch.equal(got, want)


def test_decode_linear_supported_boundaries():
    ok = OF.decode_linear_supported
    assert OF.DEC_LINEAR_KERNEL_MAX_B == 32
    assert 1 <= OF.DEC_LINEAR_MAX_B <= OF.DEC_LINEAR_KERNEL_MAX_B
    top = OF.DEC_LINEAR_MAX_B
    for dtype in (BF, F32):
        assert ok(1, 64, 16, "none", dtype)
        assert ok(top, 64, 16, "none", dtype)
        assert not ok(0, 64, 16, "none", dtype)
        assert not ok(top + 1, 64, 16, "none", dtype)
        assert not ok(33, 64, 16, "none", dtype)
        # K: whole 64-element steps
        assert ok(1, 128, 16, "gelu", dtype)
        assert not ok(1, 0, 16, "none", dtype)
        assert not ok(1, 32, 16, "none", dtype)
        assert not ok(1, 96, 16, "none", dtype)
        # N: 16-column tiles, of each half for GLU
        assert ok(1, 64, 48, "gelu", dtype)
        assert not ok(1, 64, 0, "none", dtype)
        assert not ok(1, 64, 24, "none", dtype)
        assert ok(1, 64, 32, "glu", dtype)
        assert ok(1, 64, 96, "glu", dtype)
        assert not ok(1, 64, 16, "glu", dtype)
        assert not ok(1, 64, 48, "glu", dtype)
        assert not ok(1, 64, 16, "relu", dtype)
    assert not ok(1, 64, 16, "none", torch.float16)
    assert not ok(1, 64, 16, "none", torch.float64)
    # the flagship's shapes all route
    for K, N, act in [(1536, 4608, "none"), (1536, 1536, "none"),
                      (1536, 12288, "glu"), (1536, 6144, "gelu"),
                      (3072, 3072, "none"), (6144, 1536, "none"),
                      (3072, 1536, "none"), (1536, 256, "none")]:
        assert ok(1, K, N, act, BF), (K, N, act)


def test_routing_limit_moves_the_predicate(monkeypatch):
    monkeypatch.setattr(OF, "DEC_LINEAR_MAX_B", 8)
    assert OF.decode_linear_supported(8, 64, 16, "none", BF)
    assert not OF.decode_linear_supported(9, 64, 16, "none", BF)


def test_eager_ops_tag_is_documented():
    from progen_amd.ops import dispatch
    assert "dec_linear" in dispatch.use_hip.__doc__


# ---------------------------------------------------------------------------
# the decode step and the samplers: fused_linear changes no token
# ---------------------------------------------------------------------------

def _glu_model():
    # the model of test_gpu_decode_fused.py::test_fused_decode_matches_hip_forward
    cfg = ProGenConfig(num_tokens=256, dim=128, seq_len=256, depth=3,
                       window_size=64, global_mlp_depth=1, heads=2,
                       dim_head=64)
    torch.manual_seed(5)
    return ProGenBase(cfg).eval()


def _sgu_gelu_model():
    # the model of test_gpu_decode_fused.py::_graph_model
    cfg = ProGenConfig(num_tokens=256, dim=256, depth=3, heads=4,
                       dim_head=64, window_size=64, seq_len=256,
                       ff_glu=False, global_mlp_depth=1)
    torch.manual_seed(3)
    return ProGenBase(cfg).eval()


MODELS = {"glu": _glu_model, "sgu_gelu": _sgu_gelu_model}


@pytest.fixture(scope="module", params=list(MODELS))
def model(request):
    return MODELS[request.param]()


def test_step_goes_through_decode_linear(model, monkeypatch):
    """Every projection and the logits head: 4 calls per GLU layer, 5 per
    SGU layer, 1 for the head — and none with the switch off."""
    calls = []
    real = OF.decode_linear
    monkeypatch.setattr(OF, "decode_linear",
                        lambda x, w, b=None, act="none":
                        calls.append(act) or real(x, w, b, act))
    cache = decode.DecodeCache(model, batch=2)
    pos = torch.zeros((), dtype=torch.long)
    tok = torch.tensor([3, 9])
    want = decode.forward_step_fused(model, tok, cache, pos)
    assert not calls
    cache = decode.DecodeCache(model, batch=2)
    got = decode.forward_step_fused(model, tok, cache, pos, fused_linear=True)
    n_sgu = sum(ff.sgu is not None for _, ff in model.layers)
    assert len(calls) == 4 * len(model.layers) + n_sgu + 1
    n_glu = sum(bool(ff.glu) for _, ff in model.layers)
    assert calls.count("glu") == n_glu
    assert calls.count("gelu") == len(model.layers) - n_glu
    assert torch.equal(got, want)


def test_sample_cached_fused_linear_emits_the_same_tokens(model):
    prime = torch.randint(1, 256, (5,),
                          generator=torch.Generator().manual_seed(1))
    g1 = torch.Generator().manual_seed(11)
    want = decode.sample_cached(model, prime.clone(), 40, top_k=20,
                                generator=g1, fused=True)
    g2 = torch.Generator().manual_seed(11)
    got = decode.sample_cached(model, prime.clone(), 40, top_k=20,
                               generator=g2, fused=True, fused_linear=True)
    assert torch.equal(got, want)


def test_sample_cached_batch_fused_linear_emits_the_same_tokens(model):
    g = torch.Generator().manual_seed(2)
    primes = [torch.randint(1, 256, (4,), generator=g),
              torch.randint(1, 256, (7,), generator=g)]
    want = decode.sample_cached_batch(model, primes, 24, fused=True)
    got = decode.sample_cached_batch(model, primes, 24, fused=True,
                                     fused_linear=True)
    assert torch.equal(got, want)
    g1 = torch.Generator().manual_seed(5)
    want = decode.sample_cached_batch(model, primes, 24, top_k=20,
                                      generator=g1, fused=True)
    g2 = torch.Generator().manual_seed(5)
    got = decode.sample_cached_batch(model, primes, 24, top_k=20,
                                     generator=g2, fused=True,
                                     fused_linear=True)
    assert torch.equal(got, want)


def test_fused_linear_without_fused_is_a_value_error():
    model = _glu_model()
    prime = torch.tensor([5, 6])
    with pytest.raises(ValueError, match="fused_linear"):
        decode.sample_cached(model, prime, 8, fused_linear=True)
    with pytest.raises(ValueError, match="fused_linear"):
        decode.sample_cached_batch(model, [prime], 8, fused_linear=True)
    cache = decode.DecodeCache(model, batch=1)
    with pytest.raises(ValueError, match="fused_linear"):
        decode.GraphedDecodeStep(model, cache, start_pos=0,
                                 fused_linear=True)


# ---------------------------------------------------------------------------
# CLI and serve plumbing
# ---------------------------------------------------------------------------

def test_sample_cli_flag_needs_fused():
    from click.testing import CliRunner
    import sample
    r = CliRunner().invoke(sample.main, ["--cached", "--fused-linear"])
    assert r.exit_code == 2
    assert "--fused-linear needs --fused" in r.output


def test_sample_cli_passes_the_flag(monkeypatch, tmp_path):
    from click.testing import CliRunner
    import sample
    seen = {}

    def fake_sample_cached(module, prime, length, **kw):
        seen.update(kw)
        return torch.zeros(length, dtype=torch.long)

    cfg = ProGenConfig(num_tokens=256, dim=16, depth=1, dim_head=8, heads=2,
                       window_size=8, seq_len=16, global_mlp_depth=1)
    model = ProGenBase(cfg)
    last = {"params": {k: v.detach().numpy()
                       for k, v in model.state_dict().items()},
            "next_seq_index": 0, "model_config": cfg.to_dict()}
    monkeypatch.setattr(sample, "get_checkpoint_fns",
                        lambda path: (None, lambda: last, None))
    monkeypatch.setattr(decode, "sample_cached", fake_sample_cached)
    r = CliRunner().invoke(sample.main,
                           ["--cached", "--fused", "--fused-linear"])
    assert r.exit_code == 0, r.output
    assert seen["fused"] is True and seen["fused_linear"] is True
    seen.clear()
    r = CliRunner().invoke(sample.main, ["--cached", "--fused"])
    assert r.exit_code == 0, r.output
    assert seen["fused"] is True and seen["fused_linear"] is False


def test_serve_cli_flag_needs_fused():
    pytest.importorskip("fastapi")
    from click.testing import CliRunner
    import serve
    r = CliRunner().invoke(serve.main, ["--fused-linear"])
    assert r.exit_code == 2
    assert "--fused-linear needs --fused" in r.output


def _client(**kw):
    from fastapi.testclient import TestClient
    from serve import create_app
    cfg = ProGenConfig(num_tokens=256, dim=16, depth=2, dim_head=8, heads=2,
                       window_size=8, seq_len=64, global_mlp_depth=1)
    torch.manual_seed(5)
    module = ProGenBase(cfg).eval()
    return TestClient(create_app(module, cfg, **kw))


def test_serve_info_and_generate_carry_the_flag(monkeypatch):
    pytest.importorskip("fastapi")
    assert _client().get("/info").json()["fused_linear"] is False
    assert _client(fused=True).get("/info").json()["fused_linear"] is False
    on = _client(fused=True, fused_linear=True)
    assert on.get("/info").json()["fused_linear"] is True
    with pytest.raises(ValueError):
        _client(fused_linear=True)

    calls = []
    real = OF.decode_linear
    monkeypatch.setattr(OF, "decode_linear",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    body = {"primes": ["# M", "# GA"], "num_tokens": 32, "seed": 123}
    want = _client(fused=True).post("/generate", json=body).json()
    assert not calls
    got = on.post("/generate", json=body).json()
    assert calls
    assert got["tokens"] == want["tokens"]


def test_bench_decode_flag_needs_fused():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                        "tools", "bench_decode.py")
    spec = importlib.util.spec_from_file_location("bench_decode_tool", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parse_args(["--graph", "--fused", "--fused-linear"])
    assert args.fused and args.fused_linear
    assert not mod.parse_args(["--fused"]).fused_linear
    with pytest.raises(SystemExit):
        mod.parse_args(["--fused-linear"])
