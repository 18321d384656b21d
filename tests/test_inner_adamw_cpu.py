"""optim.InnerAdamW without a GPU, on the checker backend (tests/inner_adamw_oracle_kernels.py:
dl_adamw_step restated in numpy): get_optimizer's dispatch on DILOCO_INNER_ADAMW, the lazy
device-side setup, the fused step against stock torch.optim.AdamW on CPU clones, the fallbacks
to torch's own step body, state_dict round trips with stock AdamW in both directions, and the
clip coefficient folded into the step.

Hyper-parameters are the reference's inner optimizer's (configs/optimizer/adamw.toml: lr 6e-4)
under its warm-up schedule (src/utils.py:78-85: lr * step / warmup_steps). Where stock AdamW
steps on the CPU as the reference, tests/stock_adamw.py says how θ is compared with it: this
torch build's CPU sqrt is 1 ulp off for 0.65 % of its arguments, the kernels' contract is the
correctly rounded one."""
import copy

import numpy as np
import pytest
import torch
from torch.optim.lr_scheduler import LambdaLR

import clip_restatement as cr
from inner_adamw_oracle_kernels import InnerAdamWOracleKernels
from diloco_amd import kernels, utils
from diloco_amd.optim import InnerAdamW
from diloco_amd.utils import get_optimizer, get_outer_model
from stock_adamw import StockPair, bits as _bits, ieee_sqrt

F = np.float32
HYPER = dict(lr=6e-4, betas=(0.9, 0.95), weight_decay=0.1)
SHAPES = [1, 3, 5, 4097, 0, 64, 65, 8191, 4096 * 3 + 7, 2]
SMALL = [3, 65, 0, 4097, 2]
WARMUP = 4


def _warmup(step):
    return step / WARMUP if step < WARMUP else 1.0


class _Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


ADAMW_CFG = _Cfg(type="AdamW", **HYPER)


@pytest.fixture
def oracle_backend():
    prev = kernels._DEFAULT
    k = InnerAdamWOracleKernels()
    kernels.set_default_kernels(k)
    utils._clip_cache.clear()
    yield k
    kernels._DEFAULT = prev
    utils._clip_cache.clear()


def _values(rng, shapes):
    return [rng.standard_normal(n).astype(F) for n in shapes]


def _params(values):
    return [torch.nn.Parameter(torch.from_numpy(v.copy())) for v in values]


def _grads(rng, shapes, scale=1.0):
    """Over four decades, with exact zeros."""
    out = []
    for n in shapes:
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 0, n) * scale).astype(F)
        g[::5] = 0
        out.append(g)
    return out


def _set_grads(params, grads):
    for p, g in zip(params, grads):
        p.grad = torch.from_numpy(g.copy())  # a fresh tensor every step, as after zero_grad()


def _assert_same(pa, oa, pb, ob, what):
    for i, (a, b) in enumerate(zip(pa, pb)):
        sa, sb = oa.state[a], ob.state[b]
        assert set(sa) == set(sb), (what, i)
        for key in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
            if key in sb:
                assert _bits(sa[key]) == _bits(sb[key]), (what, key, i)
        if "step" in sb:
            assert float(sa["step"]) == float(sb["step"]), (what, i)
            assert sa["step"].dtype == sb["step"].dtype and sa["step"].device.type == "cpu"
        n = int((a.detach() != b.detach()).sum())
        print(f"{what}: tensor {i} ({a.numel()} elements): theta differs in {n}")
        assert _bits(a) == _bits(b), (what, "theta", i, n)


def _adamw_calls(k):
    return [c for c in k.calls if c[0] == "adamw_step"]


def _module(shapes=((4, 3), (7,))):
    m = torch.nn.Module()
    m.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(*s)) for s in shapes])
    return m


# ---- dispatch ------------------------------------------------------------------------------
def test_get_optimizer_dispatch_on_the_knob(oracle_backend, monkeypatch):
    monkeypatch.delenv("DILOCO_OUTER_ADAMW", raising=False)
    monkeypatch.delenv("DILOCO_INNER_ADAMW", raising=False)
    inner = _module()
    outer = get_outer_model(inner)
    assert type(get_optimizer(inner, ADAMW_CFG)) is torch.optim.AdamW  # the default
    monkeypatch.setenv("DILOCO_INNER_ADAMW", "torch")
    assert type(get_optimizer(inner, ADAMW_CFG)) is torch.optim.AdamW
    monkeypatch.setenv("DILOCO_INNER_ADAMW", "fused")
    opt = get_optimizer(inner, ADAMW_CFG)
    assert type(opt) is InnerAdamW and isinstance(opt, torch.optim.AdamW)
    g = opt.param_groups[0]
    assert (g["lr"], g["betas"], g["weight_decay"], g["eps"]) == (6e-4, (0.9, 0.95), 0.1, 1e-8)
    assert all(a is b for a, b in zip(g["params"], inner.parameters()))
    assert type(get_optimizer(outer, ADAMW_CFG)) is torch.optim.AdamW  # an outer model: unaffected
    sgd = _Cfg(type="SGD", lr=0.7, momentum=0.9, nesterov=True)
    assert type(get_optimizer(inner, sgd)) is torch.optim.SGD
    monkeypatch.setenv("DILOCO_INNER_ADAMW", "hip")
    with pytest.raises(ValueError, match="DILOCO_INNER_ADAMW"):
        get_optimizer(inner, ADAMW_CFG)
    with pytest.raises(ValueError, match="DILOCO_INNER_ADAMW"):
        get_optimizer(outer, ADAMW_CFG)


def test_setup_is_lazy(oracle_backend):
    """Made on CPU parameters, the optimizer builds nothing: no tree, no arenas, no state. The
    first fused step builds its own tree over the group's numels and two zero arenas, and the
    state holds torch's CPU step tensor and views of the arenas shaped like the parameters."""
    k = oracle_backend
    m = _module(((4, 3), (0,), (70,)))
    opt = InnerAdamW(m.parameters(), **HYPER)
    assert k.trees == [] and opt._tree is None and opt._m is None and len(opt.state) == 0
    for p in m.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    assert len(k.trees) == 1 and opt._tree is k.trees[0]
    assert opt._tree.numels == [12, 0, 70]
    assert opt._m.numel() == opt._v.numel() == opt._tree.total
    assert opt._m.dtype == torch.float32
    for p, off in zip(m.parameters(), opt._tree.seg_off[:-1]):
        s = opt.state[p]
        assert set(s) == {"step", "exp_avg", "exp_avg_sq"}
        assert s["step"].dtype == torch.float32 and s["step"].dim() == 0
        assert s["step"].device.type == "cpu" and float(s["step"]) == 1.0
        assert s["exp_avg"].shape == p.shape and s["exp_avg_sq"].shape == p.shape
        for view, arena in ((s["exp_avg"], opt._m), (s["exp_avg_sq"], opt._v)):
            assert view.untyped_storage().data_ptr() == arena.untyped_storage().data_ptr()
            assert view.storage_offset() == int(off) and view.is_contiguous()
    opt.step()
    assert len(k.trees) == 1  # the optimizer keeps its tree
    assert utils._clip_cache == {}  # and never borrows the clip cache's


# ---- the fused step ------------------------------------------------------------------------
def test_four_steps_match_stock_adamw(oracle_backend):
    """Four steps under the warm-up schedule, a fresh .grad tensor per parameter every step:
    θ, exp_avg, exp_avg_sq and step bit-equal to stock AdamW(foreach=False) on CPU clones fed
    the same gradients (tests/stock_adamw.py: as shipped, and with the IEEE sqrt); one
    dl_adamw_step over the whole tree per step, without a coefficient."""
    k = oracle_backend
    rng = np.random.default_rng(31)
    vals = _values(rng, SHAPES)
    pa = _params(vals)
    oa = InnerAdamW(pa, **HYPER)
    sa = LambdaLR(oa, _warmup)
    ref = StockPair(vals, _warmup, **HYPER)
    lrs = []
    for s in range(1, 5):
        g = _grads(rng, SHAPES)
        _set_grads(pa, g)
        lrs.append(oa.param_groups[0]["lr"])
        oa.step()
        sa.step()
        ref.step(g)
        ref.check(pa, oa, f"step {s}")
        assert _adamw_calls(k) == [("adamw_step", -1)] * s
        for p, x in zip(pa, g):
            assert p.grad.numpy().tobytes() == x.tobytes()  # only read
    assert lrs == [6e-4 * i / WARMUP for i in range(4)]
    assert k.coefs == [None] * 4
    assert not [c for c in k.calls if c[0] != "adamw_step"]


# ---- fallbacks -----------------------------------------------------------------------------
def _fallback_case(why, vals):
    """(InnerAdamW, its params, stock AdamW, its params, per-step gradient hook)."""
    kw = dict(HYPER)
    pa, pb = _params(vals), _params(vals)
    skip = None
    if why == "amsgrad":
        kw["amsgrad"] = True
    elif why == "beta1":
        kw["betas"] = (0.4, 0.9)
    elif why == "tensor_lr":
        kw["lr"] = torch.tensor(6e-4)
    elif why == "bf16":
        pa[1] = torch.nn.Parameter(pa[1].detach().bfloat16())
        pb[1] = torch.nn.Parameter(pb[1].detach().bfloat16())
    elif why == "grad_none":
        skip = 2
    if why == "two_groups":
        oa = InnerAdamW([{"params": pa[:2]}, {"params": pa[2:], "lr": 1e-3}], **kw)
        ob = torch.optim.AdamW([{"params": pb[:2]}, {"params": pb[2:], "lr": 1e-3}], **kw)
    else:
        oa, ob = InnerAdamW(pa, **kw), torch.optim.AdamW(pb, **kw)
    return oa, pa, ob, pb, skip


@pytest.mark.parametrize("why", ["amsgrad", "two_groups", "beta1", "grad_none", "tensor_lr",
                                 "bf16"])
def test_fallback_is_torchs_own_step(why, oracle_backend):
    """Outside the fused pass's contract step() runs torch's own step body: three steps
    bit-equal to a stock AdamW on clones, and dl_adamw_step is never launched."""
    rng = np.random.default_rng(7)
    vals = _values(rng, SMALL)
    oa, pa, ob, pb, skip = _fallback_case(why, vals)
    for s in (1, 2, 3):
        g = _grads(rng, SMALL)
        for params in (pa, pb):
            for i, (p, x) in enumerate(zip(params, g)):
                p.grad = None if i == skip else torch.from_numpy(x.copy()).to(p.dtype)
        oa.step()
        ob.step()
        live = [i for i in range(len(pa)) if i != skip]
        _assert_same([pa[i] for i in live], oa, [pb[i] for i in live], ob, (why, s))
        if skip is not None:
            assert _bits(pa[skip]) == _bits(pb[skip]) and len(oa.state.get(pa[skip], {})) == 0
    assert oracle_backend.calls == [] and oracle_backend.trees == []


def test_state_created_by_a_fallback_is_adopted(oracle_backend):
    """A step outside the contract (amsgrad set for one step) leaves torch's own state tensors;
    the next fused step copies them into the arenas and goes on from them: the same bits as a
    stock AdamW that had amsgrad set for that one step. torch's code steps with the IEEE sqrt
    on both sides (tests/stock_adamw.py)."""
    with ieee_sqrt():
        _adopted(oracle_backend)


def _adopted(oracle_backend):
    rng = np.random.default_rng(9)
    vals = _values(rng, SMALL)
    pa, pb = _params(vals), _params(vals)
    oa, ob = InnerAdamW(pa, **HYPER), torch.optim.AdamW(pb, foreach=False, **HYPER)
    for s in (1, 2, 3):
        g = _grads(rng, SMALL)
        _set_grads(pa, g)
        _set_grads(pb, g)
        for o in (oa, ob):
            o.param_groups[0]["amsgrad"] = s == 1
        oa.step()
        ob.step()
        for p, q in zip(pa, pb):  # amsgrad's extra buffer stays in both states, unused later
            assert _bits(oa.state[p]["max_exp_avg_sq"]) == _bits(ob.state[q]["max_exp_avg_sq"])
    # the extra key keeps the state outside the contract: still torch's own step body
    assert _adamw_calls(oracle_backend) == []
    for o, params in ((oa, pa), (ob, pb)):
        for p in params:
            del o.state[p]["max_exp_avg_sq"]
    g = _grads(rng, SMALL)
    _set_grads(pa, g)
    _set_grads(pb, g)
    oa.step()
    ob.step()
    _assert_same(pa, oa, pb, ob, "adopted")
    assert _adamw_calls(oracle_backend) == [("adamw_step", -1)]
    assert all(oa.state[p]["exp_avg"] is v for p, v in zip(pa, oa._m_views))


# ---- state_dict ----------------------------------------------------------------------------
def _run(opt, params, grads):
    for g in grads:
        _set_grads(params, g)
        with ieee_sqrt():  # where the optimizer is stock AdamW (tests/stock_adamw.py)
            opt.step()


@pytest.mark.parametrize("direction", ["inner_to_inner", "inner_to_stock", "stock_to_inner"])
def test_state_dict_round_trips(direction, oracle_backend):
    """Two steps, state_dict() (copied, as a checkpoint on disk is), load_state_dict into
    another optimizer on clones of the parameters, two more steps: bit-equal to the
    uninterrupted InnerAdamW run, into a fresh InnerAdamW, into a stock AdamW, and from a
    stock AdamW into an InnerAdamW that has not stepped yet. Stock AdamW steps with the IEEE
    sqrt (tests/stock_adamw.py; test_four_steps_match_stock_adamw has the comparison with
    torch's own)."""
    rng = np.random.default_rng(11)
    vals = _values(rng, SMALL)
    grads = [_grads(rng, SMALL) for _ in range(4)]
    pu = _params(vals)
    ou = InnerAdamW(pu, **HYPER)
    _run(ou, pu, grads)  # the uninterrupted run

    p1 = _params(vals)
    first = torch.optim.AdamW(p1, foreach=False, **HYPER) if direction == "stock_to_inner" \
        else InnerAdamW(p1, **HYPER)
    _run(first, p1, grads[:2])
    sd = copy.deepcopy(first.state_dict())
    p2 = _params([p.detach().numpy() for p in p1])
    second = torch.optim.AdamW(p2, foreach=False, **HYPER) if direction == "inner_to_stock" \
        else InnerAdamW(p2, **HYPER)
    second.load_state_dict(sd)
    if isinstance(second, InnerAdamW):
        assert second._tree is None  # loading builds nothing
    _run(second, p2, grads[2:])
    _assert_same(p2, second, pu, ou, direction)
    want = {"inner_to_inner": 8, "inner_to_stock": 6, "stock_to_inner": 6}[direction]
    assert len(_adamw_calls(oracle_backend)) == want
    if isinstance(second, InnerAdamW):  # the loaded copies went into the arenas
        assert all(second.state[p]["exp_avg"] is v for p, v in zip(p2, second._m_views))
        assert all(second.state[p]["exp_avg_sq"] is v for p, v in zip(p2, second._v_views))
    # and the two state dicts are interchangeable: the same keys, shapes and dtypes
    a, b = second.state_dict(), ou.state_dict()
    drop = ("foreach",)  # the stock optimizer of these tests sets it; nothing else differs
    assert [{k: v for k, v in g.items() if k not in drop} for g in a["param_groups"]] == \
        [{k: v for k, v in g.items() if k not in drop} for g in b["param_groups"]]
    for i in b["state"]:
        assert {k: (v.shape, v.dtype) for k, v in a["state"][i].items()} == \
            {k: (v.shape, v.dtype) for k, v in b["state"][i].items()}


def test_a_deep_copy_goes_on_from_the_copied_state(oracle_backend):
    """torch copies an optimizer as (defaults, state, param_groups): the copy has no tree and
    no arenas of its own yet, adopts the copied state at its next step and matches the
    original from there on."""
    rng = np.random.default_rng(19)
    vals = _values(rng, SMALL)
    grads = [_grads(rng, SMALL) for _ in range(3)]
    pa = _params(vals)
    oa = InnerAdamW(pa, **HYPER)
    _run(oa, pa, grads[:2])
    ob = copy.deepcopy(oa)
    pb = ob.param_groups[0]["params"]
    assert ob._tree is None and ob._m is None and all(p is not q for p, q in zip(pa, pb))
    _run(oa, pa, grads[2:])
    _run(ob, pb, grads[2:])
    _assert_same(pb, ob, pa, oa, "copy")
    assert ob._tree is not oa._tree and ob._m.data_ptr() != oa._m.data_ptr()


# ---- the folded clip -----------------------------------------------------------------------
@pytest.mark.parametrize("factor", [0.5, 2.0])
def test_folded_clip_equals_clip_then_step(factor, oracle_backend):
    """opt.clip_grad_norm_(m); opt.step() against utils.clip_grad_norm_(params, m); opt.step()
    on an identical twin, with a max_norm that clips and one that does not: θ, exp_avg and
    exp_avg_sq bit-equal, the two norms bit-equal, the gradients untouched on the fold side
    (and scaled on the twin's when it clips), no dl_scale_by on the fold side."""
    k = oracle_backend
    rng = np.random.default_rng(13)
    vals = _values(rng, SHAPES)
    pa, pb = _params(vals), _params(vals)
    oa, ob = InnerAdamW(pa, **HYPER), InnerAdamW(pb, **HYPER)
    for s in (1, 2):
        g = _grads(rng, SHAPES)
        norm0, _ = cr.norm_and_coef(g, 1.0)
        max_norm = float(norm0) * factor
        _set_grads(pa, g)
        _set_grads(pb, g)
        del k.calls[:]
        na = oa.clip_grad_norm_(max_norm)
        oa.step()
        fold_calls = list(k.calls)
        nb = utils.clip_grad_norm_(pb, max_norm)
        ob.step()
        assert [c[0] for c in fold_calls] == ["grad_sumsq", "norm_finish", "adamw_step"]
        assert na.dtype == torch.float32 and na.dim() == 0
        assert _bits(na) == _bits(nb) and _bits(na)[1] == norm0.tobytes()
        assert (k.coefs[-2] < 1) == (factor < 1) and k.coefs[-1] is None
        _assert_same(pa, oa, pb, ob, (factor, s))
        _, _, clipped = cr.clip(g, max_norm)
        for p, q, x, c in zip(pa, pb, g, clipped):
            assert p.grad.numpy().tobytes() == x.tobytes()  # the fold leaves .grad unscaled
            assert q.grad.numpy().tobytes() == c.tobytes()
        assert oa._pending is None


def test_fold_errors(oracle_backend):
    """The pending coefficient belongs to the gradient tensors it was computed from: a step
    that finds other tensors, or that cannot take the fused pass, raises and steps nothing;
    zero_grad() drops it; error_if_nonfinite raises torch's error and leaves nothing pending."""
    rng = np.random.default_rng(15)
    vals = _values(rng, SMALL)
    pa = _params(vals)
    oa = InnerAdamW(pa, **HYPER)
    _set_grads(pa, _grads(rng, SMALL))
    oa.clip_grad_norm_(1e-3)
    _set_grads(pa, _grads(rng, SMALL))  # other tensors
    with pytest.raises(RuntimeError, match="gradient tensors"):
        oa.step()
    assert _adamw_calls(oracle_backend) == [] and oa._pending is None
    assert all(p.detach().numpy().tobytes() == v.tobytes() for p, v in zip(pa, vals))

    oa.clip_grad_norm_(1e-3)
    oa.param_groups[0]["amsgrad"] = True  # outside the contract: torch's body cannot apply it
    with pytest.raises(RuntimeError, match="pending"):
        oa.step()
    oa.param_groups[0]["amsgrad"] = False
    assert all(p.detach().numpy().tobytes() == v.tobytes() for p, v in zip(pa, vals))

    oa.clip_grad_norm_(1e-3)
    assert oa._pending is not None
    oa.zero_grad()
    assert oa._pending is None and all(p.grad is None for p in pa)
    _set_grads(pa, _grads(rng, SMALL))
    oa.step()
    assert oracle_backend.coefs == [None]

    g = _grads(rng, SMALL)
    g[1][3] = np.inf
    _set_grads(pa, g)
    with pytest.raises(RuntimeError, match="non-finite"):
        oa.clip_grad_norm_(1.0, error_if_nonfinite=True)
    assert oa._pending is None


def test_clip_outside_the_contract_is_the_plain_clip(oracle_backend):
    """When the fused pass does not apply, InnerAdamW.clip_grad_norm_ is utils.clip_grad_norm_:
    the gradients are scaled in place and nothing stays pending."""
    rng = np.random.default_rng(17)
    vals = _values(rng, SMALL)
    pa, pb = _params(vals), _params(vals)
    oa = InnerAdamW(pa, amsgrad=True, **HYPER)
    g = _grads(rng, SMALL)
    _set_grads(pa, g)
    _set_grads(pb, g)
    na = oa.clip_grad_norm_(1e-3)
    nb = utils.clip_grad_norm_(pb, 1e-3)
    assert _bits(na) == _bits(nb) and oa._pending is None
    assert all(_bits(p.grad) == _bits(q.grad) for p, q in zip(pa, pb))
    assert any(p.grad.numpy().tobytes() != x.tobytes() for p, x in zip(pa, g))
    oa.step()  # torch's own body, on the scaled gradients
    assert _adamw_calls(oracle_backend) == []
