"""The top-k wire's 4-bit values without a GPU: symbols, argument errors, get_outer_model's knob."""
import pytest
import torch

from diloco_amd import _lib
from diloco_amd.utils import _TOPK_VALUES, get_outer_model
from test_topk_cpu import _calls


def test_topk_fp4_abi_and_knob(monkeypatch):
    lib = _lib.load()
    assert (_lib.TOPK_FP4_SLOT_BYTES(64), _lib.TOPK_FP4_SLOT_BYTES(256)) == (144, 528)
    for k in (12, 264):
        for name, args in _calls(k).items():
            name = name.replace("topk", "topk_fp4")
            assert hasattr(lib, name)
            with pytest.raises(_lib.DilocoHipError, match=r"%s: k %d\b" % (name, k)) as e:
                _lib.call(name, *args)
            assert e.value.code == -1
    inner = torch.nn.Linear(3, 2)
    for v in ("DILOCO_OUTER_WIRE", "DILOCO_OUTER_TOPK", "DILOCO_OUTER_TOPK_VALUES"):
        monkeypatch.delenv(v, raising=False)
    dev = dict(placement="device")
    assert getattr(get_outer_model(inner, wire="topk", **dev), _TOPK_VALUES) == "f32"
    assert getattr(get_outer_model(inner, wire="topk", topk_values="fp4", **dev), _TOPK_VALUES) == "fp4"
    monkeypatch.setenv("DILOCO_OUTER_TOPK_VALUES", "fp4")
    assert getattr(get_outer_model(inner, wire="topk", **dev), _TOPK_VALUES) == "fp4"
    for wire in ("f32", "bf16", "int8", "fp4"):  # the variable is consulted for its own wire only
        assert getattr(get_outer_model(inner, wire=wire, **dev), _TOPK_VALUES) == "f32"
        with pytest.raises(ValueError, match="topk_values"):
            get_outer_model(inner, wire=wire, topk_values="fp4", **dev)
    with pytest.raises(ValueError, match="topk_values 'int4'"):
        get_outer_model(inner, wire="topk", topk_values="int4", **dev)
