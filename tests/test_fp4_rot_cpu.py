"""The rotated fp4 wire, without a GPU: the C-ABI carries the four entry points at the same
version, argument errors come before any device work, and the rotate knob is the fp4 wire's."""
import os
import re

import pytest
import torch

from conftest import REPO
from diloco_amd import _lib

ENTRY_POINTS = (("dl_delta_fp4_rot", 8), ("dl_unpack_sgd_fp4_rot", 12),
                ("dl_unpack_adamw_fp4_rot", 16), ("dl_decode_fp4_rot", 6))


def test_abi_declares_the_rot_entry_points_at_version_8():
    with open(os.path.join(REPO, "include", "diloco_hip.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name, nargs in ENTRY_POINTS:
        assert re.search(r"DL_API\s+int\s+" + name + r"\s*\(", header), name
        assert len(_lib.SIGNATURES[name][1]) == nargs and hasattr(lib, name)
    assert lib.dl_abi_version() == 8


def test_argument_checks_come_before_the_device():
    E = _lib.DilocoHipError
    sgd, adam = (0.7, 0.9, 1, 0, -1, None), (1.0, 0.1, 0.95, 0.05, -0.1, 1.0, 1e-8, -1, None)
    for name, args in [("dl_delta_fp4_rot", (0, 64, None, 7, 192, None)),
                       ("dl_unpack_sgd_fp4_rot", (64, 7, 128, 192) + sgd),
                       ("dl_unpack_adamw_fp4_rot", (64, 7, 128, 192, 256) + adam),
                       ("dl_decode_fp4_rot", (64, 7, 128, None))]:
        with pytest.raises(E, match="null tree") as e:
            _lib.call(name, None, 0, *args)
        assert e.value.code == -1 and name in str(e.value)  # DL_E_ARG
    # dl_decode_fp4_rot checks its pointers before the tree, as dl_gather_fp4 does
    for args, msg, code in [((None, 7, 128), "slots is null", -1), ((64, 7, None), "dst is null", -1),
                            ((72, 7, 128), "slots not 16-B", -3), ((64, 7, 132), "dst not 16-B", -3)]:
        with pytest.raises(E, match=msg) as e:
            _lib.call("dl_decode_fp4_rot", None, _lib.ALL_BUCKETS, *args, None)
        assert e.value.code == code  # DL_E_ARG / DL_E_ALIGN


def test_rotate_is_the_fp4_wires_knob(monkeypatch):
    from diloco_amd.utils import _ROTATE, get_outer_model

    def model():
        m = torch.nn.Module()
        m.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(8))])
        return m
    for v in ("DILOCO_OUTER_WIRE", "DILOCO_OUTER_FP4_ROTATE", "DILOCO_OUTER_FP4_SEED"):
        monkeypatch.delenv(v, raising=False)
    with pytest.raises(ValueError, match="rotate"):
        get_outer_model(model(), wire="int8", rotate=True)
    assert getattr(get_outer_model(model(), wire="fp4"), _ROTATE) is None  # default off
    assert getattr(get_outer_model(model(), wire="fp4", rotate=True), _ROTATE) == 0x5EED
    monkeypatch.setenv("DILOCO_OUTER_FP4_ROTATE", "1")
    monkeypatch.setenv("DILOCO_OUTER_FP4_SEED", "0x1234")
    assert getattr(get_outer_model(model(), wire="fp4"), _ROTATE) == 0x1234
    assert getattr(get_outer_model(model(), wire="int8"), _ROTATE) is None  # its own wire only
