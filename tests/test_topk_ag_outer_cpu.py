"""The outer step on the gathered top-k slots without a GPU: symbols, argument, knob."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import PKG
from diloco_amd import _lib
from diloco_amd.utils import get_outer_model

ATTR = "_diloco_topk_exchange"


@pytest.mark.parametrize("symbol,nargs", [("dl_unpack_sgd_topk_ag", 14), ("dl_unpack_sgd_topk_fp4_ag", 14),
                                          ("dl_unpack_adamw_topk_ag", 18), ("dl_unpack_adamw_topk_fp4_ag", 18)])
def test_the_symbols_resolve_with_the_declared_argument_counts(symbol, nargs):
    assert hasattr(_lib.load(), symbol) and len(_lib.SIGNATURES[symbol][1]) == nargs


@pytest.mark.parametrize("kw", [dict(wire="topk", topk_exchange="scatter"),
                                dict(wire="fp4", topk_exchange="gather"),
                                dict(topk_exchange="gather")])
def test_topk_exchange_is_checked_before_anything_is_built(kw):
    with pytest.raises(ValueError, match="topk_exchange"):
        get_outer_model(torch.nn.Linear(3, 2), **kw)


def test_the_knob_parses_for_its_own_wire_and_defaults_to_reduce(monkeypatch):
    monkeypatch.delenv("DILOCO_OUTER_TOPK_EXCHANGE", raising=False)
    assert getattr(get_outer_model(torch.nn.Linear(3, 2), wire="topk"), ATTR) == "reduce"
    assert getattr(get_outer_model(torch.nn.Linear(3, 2), wire="topk", topk_exchange="gather"), ATTR) == "gather"
    code = ("import torch; from diloco_amd.utils import get_outer_model as g; m = torch.nn.Linear(3, 2); "
            f"print(getattr(g(m, wire='topk'), {ATTR!r}), getattr(g(m, wire='fp4'), {ATTR!r}))")
    env = dict(os.environ, DILOCO_OUTER_TOPK_EXCHANGE="gather", PYTHONPATH=PKG)
    run = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True)
    assert run.stdout.split() == ["gather", "reduce"]
