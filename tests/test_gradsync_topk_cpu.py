"""The top-k wire of the per-step DP gradient sync without a GPU: the four C-ABI entry points and
their check of k, GradSync's topk / topk_values / error_feedback arguments and the DILOCO_DP_TOPK*
knobs. The kernels' results are checked on the GPU (tests/test_gradsync_topk_gpu.py)."""
import os
import re
import subprocess
import sys

import pytest
import torch

from clip_oracle_kernels import as_params
from conftest import PKG, REPO
from diloco_amd import _lib, comm, kernels
from diloco_amd.gradsync import SLOT_WIRES, GradSync, slot_wire_bytes
from gradsync_fp4_inputs import groupwise
from gradsync_fp4_oracle_kernels import GradSyncFp4OracleKernels

GATHER = ("dl_gather_topk", "dl_gather_topk_fp4")
UNPACK = ("dl_unpack_avg_topk", "dl_unpack_avg_topk_fp4")


def _calls(k):
    """Every new entry point with good buffers (addresses only) and a null tree."""
    return [(n, (None, 0, 1, 128, k, 64, None)) for n in GATHER] + \
           [(n, (None, 0, 64, k, 1, 136, None)) for n in UNPACK]


def test_abi_entry_points_and_their_argument_checks():
    with open(os.path.join(REPO, "include", "diloco_hip.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name, _args in _calls(64):
        assert re.search(r"DL_API\s+int\s+" + name + r"\s*\(", header), name
        assert len(_lib.SIGNATURES[name][1]) == 7 and hasattr(lib, name), name
    for m in ("gather_topk", "gather_topk_fp4", "unpack_avg_topk", "unpack_avg_topk_fp4"):
        assert callable(getattr(kernels.HipKernels, m))
    for k in (0, 7, 12, 264):  # DL_E_ARG, the message names the call and k
        for name, args in _calls(k):
            with pytest.raises(_lib.DilocoHipError, match=r"%s: k %d\b" % (name, k)) as e:
                _lib.call(name, *args)
            assert e.value.code == -1
    for name, args in _calls(64):  # good k and buffers: the null tree is what is reported
        with pytest.raises(_lib.DilocoHipError, match="null tree"):
            _lib.call(name, *args)


def _gs(**kw):
    return GradSync(as_params(groupwise(1)), None, 1, kernels=GradSyncFp4OracleKernels(), **kw)


def test_gradsync_arguments():
    gs = _gs(wire_dtype="topk")
    assert gs.topk_wire and (gs.topk, gs.topk_values, gs.slot_bytes) == (64, "f32", 384)
    assert gs.error_feedback and gs.q_residual is not None  # None means ON for this wire only
    assert not _gs(wire_dtype="topk", error_feedback=False).error_feedback
    gs = _gs(wire_dtype="topk", topk=256, topk_values="fp4")
    assert (gs.topk, gs.topk_values, gs.slot_bytes) == (256, "fp4", 16 + 512)
    assert gs.q_slots.numel() == gs.tree.n_chunks * 528
    assert slot_wire_bytes("topk", 8, "f32") == 48 and slot_wire_bytes("topk", 8, "fp4") == 32
    for wire in (torch.float32, torch.bfloat16, torch.int8, "fp4"):  # the others are as they were
        gs = _gs(wire_dtype=wire)
        assert not gs.topk_wire and gs.topk is None and not gs.error_feedback
        assert gs.slot_bytes == slot_wire_bytes(wire) == SLOT_WIRES.get(wire)
        with pytest.raises(ValueError, match="topk=64 is the 'topk' wire's"):
            _gs(wire_dtype=wire, topk=64)
        with pytest.raises(ValueError, match="topk_values='fp4' is how the 'topk' wire"):
            _gs(wire_dtype=wire, topk_values="fp4")
    for k in (0, 12, 264):
        with pytest.raises(ValueError, match="topk %d: a multiple of 8" % k):
            _gs(wire_dtype="topk", topk=k)
    with pytest.raises(ValueError, match="topk_values 'int4'"):
        _gs(wire_dtype="topk", topk_values="int4")
    with pytest.raises(ValueError, match="topk wire has its own rank-order exchange.*a2a"):
        _gs(wire_dtype="topk", exchange="a2a")


def test_dp_knobs(monkeypatch):
    assert comm.DP_WIRES["topk"] == "topk"
    monkeypatch.setattr(comm, "DP_WIRE", "topk")
    monkeypatch.setattr(comm, "DP_Q8_EF", False)
    monkeypatch.setattr(comm, "DP_FP4_EF", False)
    for ef in (True, False):
        monkeypatch.setattr(comm, "DP_TOPK_EF", ef)
        assert comm.dp_wire() == ("topk", ef)
    monkeypatch.setattr(comm, "DP_TOPK", 128)
    monkeypatch.setattr(comm, "DP_TOPK_VALUES", "fp4")
    assert comm.dp_topk() == {"topk": 128, "topk_values": "fp4"}
    gs = _gs(wire_dtype=comm.dp_wire()[0], error_feedback=comm.dp_wire()[1], **comm.dp_topk())
    assert (gs.topk, gs.topk_values, gs.error_feedback) == (128, "fp4", False)
    monkeypatch.setattr(comm, "DP_TOPK_EF", True)
    for wire in ("f32", "bf16", "int8", "fp4"):  # consulted for this wire only
        monkeypatch.setattr(comm, "DP_WIRE", wire)
        assert comm.dp_wire()[1] is False and comm.dp_topk() == {}


def test_dp_knobs_from_the_environment():
    env = {k: v for k, v in os.environ.items() if not k.startswith("DILOCO_DP_")}
    env["PYTHONPATH"] = os.pathsep.join([PKG, REPO])
    code = ("from diloco_amd import comm; "
            "print(comm.DP_TOPK, comm.DP_TOPK_VALUES, comm.DP_TOPK_EF, *comm.dp_wire())")

    def run():
        return subprocess.run([sys.executable, "-c", code], env=env, check=True,
                              capture_output=True, text=True, timeout=120).stdout.split()

    assert run() == ["64", "f32", "True", "torch.float32", "False"]
    env.update(DILOCO_DP_WIRE="topk")
    assert run() == ["64", "f32", "True", "topk", "True"]
    env.update(DILOCO_DP_TOPK="32", DILOCO_DP_TOPK_VALUES="fp4", DILOCO_DP_TOPK_EF="0")
    assert run() == ["32", "fp4", "False", "topk", "False"]
