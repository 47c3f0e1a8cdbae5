"""serve.py with ``device_sampling=True``: the flag is reported by /info,
requests decode through ``OF.decode_sample`` (CPU: its reference), a
request's seed keys the sampler's stream, and greedy requests return the
tokens of the host sampler."""

import pytest
import torch

fastapi = pytest.importorskip("fastapi")
from fastapi.testclient import TestClient  # noqa: E402

from progen_amd import ProGenBase, ProGenConfig  # noqa: E402
from serve import create_app  # noqa: E402


def _client(**kw):
    cfg = ProGenConfig(num_tokens=256, dim=16, depth=2, dim_head=8, heads=2,
                       window_size=8, seq_len=64, global_mlp_depth=1)
    torch.manual_seed(5)
    module = ProGenBase(cfg).eval()
    return TestClient(create_app(module, cfg, **kw))


def test_info_reports_device_sampling():
    assert _client().get("/info").json()["device_sampling"] is False
    assert _client(device_sampling=True).get("/info").json()[
        "device_sampling"] is True


def test_greedy_generate_matches_the_host_sampler(monkeypatch):
    from progen_amd.ops import functional as OF
    calls = []
    real = OF.decode_sample
    monkeypatch.setattr(OF, "decode_sample",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    body = {"primes": ["# M", "# GA"], "num_tokens": 48, "top_k": 0}
    want = _client().post("/generate", json=body).json()
    assert not calls
    for kw in (dict(), dict(fused=True, fused_linear=True)):
        got = _client(device_sampling=True, **kw).post(
            "/generate", json=body).json()
        assert calls
        assert got["tokens"] == want["tokens"]
        assert got["sequences"] == want["sequences"]


def test_seed_keys_the_device_stream():
    on = _client(device_sampling=True)
    body = {"primes": ["# M", "# GA"], "num_tokens": 48, "seed": 123}
    a = on.post("/generate", json=body).json()["tokens"]
    assert on.post("/generate", json=body).json()["tokens"] == a
    assert on.post("/generate", json=dict(body, seed=124)).json()["tokens"] != a
    # the decoder's own output for that seed
    from progen_amd.data import encode_tokens
    from progen_amd.decode import sample_cached_batch
    torch.manual_seed(5)
    cfg = ProGenConfig(num_tokens=256, dim=16, depth=2, dim_head=8, heads=2,
                       window_size=8, seq_len=64, global_mlp_depth=1)
    module = ProGenBase(cfg).eval()
    rows = [torch.tensor([0] + encode_tokens(p)) for p in body["primes"]]
    out = sample_cached_batch(module, rows, 48, top_k=25,
                              device_sampling=True, seed=123)
    assert a == [out[i, len(r):].tolist() for i, r in enumerate(rows)]


def test_missing_seed_is_drawn_on_the_host_and_bad_seed_is_refused():
    on = _client(device_sampling=True)
    body = {"primes": ["# M"], "num_tokens": 32}
    torch.manual_seed(1)
    a = on.post("/generate", json=body)
    assert a.status_code == 200
    torch.manual_seed(1)
    assert on.post("/generate", json=body).json()["tokens"] == a.json()["tokens"]
    assert on.post("/generate", json=dict(body, seed=-1)).status_code == 400
    assert on.post("/generate",
                   json=dict(body, seed=2 ** 63)).status_code == 400
