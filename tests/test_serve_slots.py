"""serve.py with ``slots=N``: /info reports it, /generate goes through one
started ``SlotEngine`` and returns what the one-request-at-a-time app
returns, a request's seed reproduces, and the option is refused without the
fused step and the device sampler, or together with prefill."""

import pytest
import torch

fastapi = pytest.importorskip("fastapi")
from click.testing import CliRunner  # noqa: E402
from fastapi.testclient import TestClient  # noqa: E402

import serve  # noqa: E402
from progen_amd import ProGenBase, ProGenConfig  # noqa: E402
from serve import create_app  # noqa: E402

ON = dict(fused=True, device_sampling=True)


def _client(**kw):
    cfg = ProGenConfig(num_tokens=256, dim=16, depth=2, dim_head=8, heads=2,
                       window_size=8, seq_len=64, global_mlp_depth=1)
    torch.manual_seed(5)
    module = ProGenBase(cfg).eval()
    return TestClient(create_app(module, cfg, **kw))


def test_info_reports_slots():
    assert _client().get("/info").json()["slots"] == 0
    with _client(slots=2, **ON) as on:
        assert on.get("/info").json()["slots"] == 2


def test_greedy_generate_equals_the_app_without_slots(monkeypatch):
    from progen_amd.ops import functional as OF
    calls = []
    real = OF.decode_sample_slots
    monkeypatch.setattr(OF, "decode_sample_slots",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    # three rows on two slots: one of them waits for a slot
    body = {"primes": ["# M", "# GA", "# K"], "num_tokens": 48, "top_k": 0}
    want = _client(**ON).post("/generate", json=body).json()
    assert not calls
    for kw in (dict(), dict(fused_linear=True)):
        with _client(slots=2, **ON, **kw) as on:
            got = on.post("/generate", json=body).json()
        assert calls
        assert got["tokens"] == want["tokens"]
        assert got["sequences"] == want["sequences"]


def test_a_requests_seed_reproduces_and_parameters_are_per_request():
    with _client(slots=2, **ON) as on:
        body = {"primes": ["# M", "# GA"], "num_tokens": 48, "seed": 123}
        a = on.post("/generate", json=body).json()["tokens"]
        # a request of another length and top_k in between
        other = on.post("/generate", json={"prime": "# K", "num_tokens": 20,
                                           "top_k": 3, "seed": 5})
        assert other.status_code == 200
        assert len(other.json()["tokens"][0]) <= 20
        assert on.post("/generate", json=body).json()["tokens"] == a
        assert on.post("/generate",
                       json=dict(body, seed=124)).json()["tokens"] != a
        # the decoder's own output for that seed
        want = _client(**ON).post("/generate", json=body).json()["tokens"]
        assert a == want
        # what the app refuses today is still refused
        assert on.post("/generate", json=dict(body, seed=-1)).status_code == 400
        assert on.post("/generate",
                       json=dict(body, num_tokens=65)).status_code == 400
        assert on.post("/generate", json={"num_tokens": 8}).status_code == 400


def test_slots_need_the_fused_step_and_the_device_sampler():
    for kw in (dict(), dict(fused=True), dict(device_sampling=True)):
        with pytest.raises(ValueError, match="slots needs"):
            _client(slots=2, **kw)
    with pytest.raises(ValueError, match="prefill"):
        _client(slots=2, prefill=True, **ON)
    with pytest.raises(ValueError, match="slots"):
        _client(slots=-1, **ON)


@pytest.mark.parametrize("argv,what", [
    (["--slots", "2"], "--slots needs"),
    (["--slots", "2", "--fused"], "--slots needs"),
    (["--slots", "2", "--device-sampling"], "--slots needs"),
    (["--slots", "2", "--fused", "--device-sampling", "--prefill"],
     "--prefill"),
])
def test_the_command_line_refuses_them_with_a_usage_error(argv, what):
    r = CliRunner().invoke(serve.main, argv)   # stops before any checkpoint
    assert r.exit_code == 2, r.output
    assert "Usage:" in r.output and what in r.output
