"""The extension loader of progen_amd/ops/dispatch.py: one table, one cache,
and the public ``ext_*`` / ``has_ext_*`` pairs on top of them (CPU; the
extensions must be built, as for the contract tests)."""

import importlib
import sys

import pytest
import torch

from progen_amd.ops import dispatch

# key of EXTENSIONS -> its public pair
PUBLIC = {
    "main": (dispatch.ext, dispatch.has_ext),
    "decode": (dispatch.ext_decode, dispatch.has_ext_decode),
    "decode_linear": (dispatch.ext_decode_linear,
                      dispatch.has_ext_decode_linear),
    "decode_sample": (dispatch.ext_decode_sample,
                      dispatch.has_ext_decode_sample),
    "prefill": (dispatch.ext_prefill, dispatch.has_ext_prefill),
    "decode_slots": (dispatch.ext_decode_slots, dispatch.has_ext_decode_slots),
}


def test_every_extension_has_its_public_pair():
    assert set(PUBLIC) == set(dispatch.EXTENSIONS)


@pytest.mark.parametrize("key", sorted(PUBLIC))
def test_public_pair_agrees_with_the_table(key):
    ext, has_ext = PUBLIC[key]
    assert has_ext() is True
    mod = ext()
    assert mod.__name__ == dispatch.EXTENSIONS[key]
    assert mod is sys.modules[dispatch.EXTENSIONS[key]]
    assert mod is ext()


def test_missing_module_raises_and_is_tried_once(monkeypatch):
    name = "progen_amd._C_no_such_module"
    monkeypatch.setitem(dispatch.EXTENSIONS, "absent", name)
    monkeypatch.setattr(dispatch, "_LOADED", dict(dispatch._LOADED))
    calls = []
    real = importlib.import_module

    def counting(mod, *a, **kw):
        calls.append(mod)
        return real(mod, *a, **kw)

    monkeypatch.setattr(dispatch.importlib, "import_module", counting)
    assert dispatch._available("absent") is False
    for _ in range(2):
        with pytest.raises(RuntimeError) as ei:
            dispatch._load("absent")
        msg = str(ei.value)
        assert name in msg, msg
        assert "ModuleNotFoundError" in msg and "No module named" in msg, msg
        assert "`python setup.py build_ext --inplace`" in msg, msg
        assert "PYTORCH_ROCM_ARCH=gfx950" in msg, msg
    assert calls == [name]


def test_use_hip_of_a_cpu_tensor_is_false():
    assert dispatch.use_hip(torch.zeros(1)) is False
    assert dispatch.use_hip(torch.zeros(1), "dec_attn") is False
