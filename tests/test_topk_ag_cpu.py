"""The all-gather exchange of the top-k wires without a GPU: symbols, argument, knob."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import PKG
from diloco_amd import _lib, comm
from diloco_amd.gradsync import GradSync


@pytest.mark.parametrize("kw", [dict(wire_dtype="fp4", topk_exchange="gather"),
                                dict(topk_exchange="reduce"),
                                dict(wire_dtype="topk", topk_exchange="scatter")])
def test_topk_exchange_is_checked_before_anything_is_built(kw):
    with pytest.raises(ValueError, match="topk_exchange"):
        GradSync([torch.nn.Parameter(torch.zeros(8))], None, 1, kernels=object(), **kw)


def test_the_symbols_resolve_and_the_knob_parses_and_defaults_to_reduce(monkeypatch):
    for symbol in ("dl_unpack_avg_topk_ag", "dl_unpack_avg_topk_fp4_ag"):
        assert symbol in _lib.SIGNATURES and hasattr(_lib.load(), symbol)
    monkeypatch.setattr(comm, "DP_WIRE", "topk")
    assert comm.DP_TOPK_EXCHANGE == "reduce" and "topk_exchange" not in comm.dp_topk()
    monkeypatch.setattr(comm, "DP_TOPK_EXCHANGE", "gather")
    assert comm.dp_topk()["topk_exchange"] == "gather"
    code = "from diloco_amd import comm; print(comm.DP_TOPK_EXCHANGE)"
    env = dict(os.environ, DILOCO_DP_TOPK_EXCHANGE="gather", PYTHONPATH=PKG)
    run = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True)
    assert run.stdout.strip() == "gather"
