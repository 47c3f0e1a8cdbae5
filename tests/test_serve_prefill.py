"""serve.py and sample.py with ``prefill``: the flag is reported by /info,
requests build the cache of their common prime prefix through
``decode.prefill`` (CPU: the reference ops) and return the tokens of the
step loop."""

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


def test_info_reports_prefill():
    assert _client().get("/info").json()["prefill"] is False
    assert _client(prefill=True).get("/info").json()["prefill"] is True


def test_greedy_generate_matches_the_step_loop(monkeypatch):
    from progen_amd.ops import functional as OF
    calls = []
    real = OF.prefill_attention
    monkeypatch.setattr(OF, "prefill_attention",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    body = {"primes": ["# MKV", "# GAMMA"], "num_tokens": 48, "top_k": 0}
    want = _client().post("/generate", json=body).json()
    assert not calls
    for kw in (dict(), dict(fused=True, fused_linear=True),
               dict(device_sampling=True)):
        del calls[:]
        got = _client(prefill=True, **kw).post("/generate", json=body).json()
        assert len(calls) == 2      # one forward: once per layer
        assert got["tokens"] == want["tokens"]
        assert got["sequences"] == want["sequences"]


def test_sample_cli_prefill_prints_the_step_loops_sample(tmp_path):
    """sample.py on a checkpoint: --cached --prefill prints what --cached
    prints (same seed, so the same gumbel draws)."""
    from click.testing import CliRunner
    import sample
    from progen_amd.checkpoint import get_checkpoint_fns, tensors_to_numpy
    cfg = ProGenConfig(num_tokens=256, dim=16, depth=2, dim_head=8, heads=2,
                       window_size=16, seq_len=64, global_mlp_depth=1)
    torch.manual_seed(5)
    module = ProGenBase(cfg)
    _, _, save = get_checkpoint_fns(str(tmp_path))
    save({"next_seq_index": 0, "model_config": cfg.to_dict(),
          "params": tensors_to_numpy(
              {k: v.detach() for k, v in module.state_dict().items()})})
    args = ["--checkpoint_path", str(tmp_path), "--prime", "# MKVL",
            "--cached"]
    want = CliRunner().invoke(sample.main, args)
    assert want.exit_code == 0, want.output
    got = CliRunner().invoke(sample.main, args + ["--prefill"])
    assert got.exit_code == 0, got.output
    assert got.output == want.output


def test_sample_cli_wants_cached_with_prefill():
    from click.testing import CliRunner
    import sample
    res = CliRunner().invoke(sample.main, ["--prefill"])
    assert res.exit_code == 2
    assert "--prefill needs --cached" in res.output
