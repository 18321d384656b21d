"""The top-k wire without a GPU: symbols and constants, argument errors, get_outer_model's knobs."""
import re

import pytest
import torch

from diloco_amd import _lib
from diloco_amd.utils import _Q8_EF, _TOPK, get_outer_model
from test_abi import HEADER

NAMES = ("dl_delta_topk", "dl_topk_reduce", "dl_unpack_sgd_topk", "dl_unpack_adamw_topk")
ADAM = (0.999, 0.1, 0.95, 0.05, -0.01, 1.0, 1e-8)


def _calls(k, ptr=16, tree=None):
    return {"dl_delta_topk": (tree, 0, 0, ptr, None, k, ptr, None),
            "dl_topk_reduce": (ptr, 2, 1, 2, None, k, 32, None),
            "dl_unpack_sgd_topk": (tree, 0, ptr, k, ptr, ptr, 0.7, 0.9, 1, 0, -1, None),
            "dl_unpack_adamw_topk": (tree, 0, ptr, k, ptr, ptr, ptr, *ADAM, -1, None)}


def test_topk_abi_and_knobs(monkeypatch):
    src = open(HEADER).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"DL_API int %s\(" % name, src) and name in _lib.SIGNATURES
        assert hasattr(lib, name)
    consts = dict(re.findall(r"#define (DL_TOPK_M\w+) (\d+)", src))
    assert (int(consts["DL_TOPK_MIN_K"]), int(consts["DL_TOPK_MAX_K"])) == (8, 256) == \
        (_lib.TOPK_MIN_K, _lib.TOPK_MAX_K)
    assert "#define DL_TOPK_SLOT_BYTES(k) (6 * (k))" in src and _lib.TOPK_SLOT_BYTES(64) == 384
    assert lib.dl_abi_version() == 8
    for k in (7, 12, 264):
        for name, args in _calls(k).items():
            with pytest.raises(_lib.DilocoHipError, match=r"\bk %d\b" % k) as e:
                _lib.call(name, *args)
            assert e.value.code == -1
    for name, args in _calls(64).items():
        if name != "dl_topk_reduce":
            with pytest.raises(_lib.DilocoHipError, match="null tree"):
                _lib.call(name, *args)
    for args, msg in [((None, 1, 1, 1, None, 64, 16, None), "recv is null"),
                      ((16, 1, 1, 1, None, 64, 20, None), "out not 16-B aligned"),
                      ((16, 1, 1, 1, 24, 64, 16, None), "residual not 16-B aligned"),
                      ((16, 0, 1, 1, None, 64, 16, None), "n 0")]:
        with pytest.raises(_lib.DilocoHipError, match=msg):
            _lib.call("dl_topk_reduce", *args)

    inner = torch.nn.Linear(3, 2)
    for v in ("DILOCO_OUTER_WIRE", "DILOCO_OUTER_TOPK", "DILOCO_OUTER_TOPK_EF"):
        monkeypatch.delenv(v, raising=False)
    m = get_outer_model(inner, placement="device", wire="topk")
    assert getattr(m, _TOPK) == 64 and getattr(m, _Q8_EF) is True  # EF defaults on, this wire only
    assert getattr(get_outer_model(inner, placement="device", wire="topk",
                                   error_feedback=False), _Q8_EF) is False
    monkeypatch.setenv("DILOCO_OUTER_TOPK_EF", "0")
    monkeypatch.setenv("DILOCO_OUTER_TOPK", "128")
    monkeypatch.setenv("DILOCO_OUTER_WIRE", "topk")
    m = get_outer_model(inner, placement="device")
    assert getattr(m, _TOPK) == 128 and getattr(m, _Q8_EF) is False
    monkeypatch.setenv("DILOCO_OUTER_TOPK_EF", "1")
    for wire in ("f32", "bf16", "int8", "fp4"):  # the variable is consulted for its own wire only
        assert getattr(get_outer_model(inner, placement="device", wire=wire), _Q8_EF) is False
    with pytest.raises(ValueError, match="topk 12"):
        get_outer_model(inner, placement="device", wire="topk", topk=12)
