"""OuterAdamW without a GPU: the arithmetic contract of the fused AdamW kernels pinned against
torch's CPU AdamW, get_optimizer's dispatch on DILOCO_OUTER_ADAMW, the reference's four calls
(src/train.py:263-269) through the mirrors' adamw_step on a numpy stand-in for the two kernels
(tests/adamw_oracle_kernels.py), the state_dict round trip through a stock AdamW, and the
fallback to torch's own step body."""
import copy
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist

from adamw_oracle_kernels import AdamWOracleKernels
from adamw_restatement import AdamWState, F, fmaf, libm_fmaf
from conftest import normwise_ok
from diloco_amd import kernels, synth
from diloco_amd.optim import OuterAdamW
from diloco_amd.trees import get_tree
from diloco_amd.utils import (compute_pseudo_gradient, get_optimizer, get_outer_model,
                              sync_inner_model)

HYPER = dict(lr=0.01, betas=(0.9, 0.95), weight_decay=0.1)


class _Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


ADAMW_CFG = _Cfg(type="AdamW", **HYPER)


def test_vector_fmaf_is_libm_fmaf():
    """The restatement's vectorised fma is exact: equal to libm's fmaf on random operands, on
    products that cancel against the addend, and on sums that land on an fp32 rounding tie."""
    rng = np.random.default_rng(0)
    n = 20000
    a = (rng.standard_normal(n) * 10.0 ** rng.uniform(-20, 20, n)).astype(F)
    b = (rng.standard_normal(n) * 10.0 ** rng.uniform(-20, 20, n)).astype(F)
    c = (rng.standard_normal(n) * 10.0 ** rng.uniform(-30, 30, n)).astype(F)
    with np.errstate(all="ignore"):  # near-total cancellation (some products overflow fp32)
        c[::3] = (-(a[::3].astype(np.float64) * b[::3])).astype(F)
    # ties: a*b = 1 + 2^-24 + 2^-30 exactly needs all 48 bits; c pushes it across the midpoint
    a[1::5], b[1::5] = F(1 + 2.0 ** -12), F(1 + 2.0 ** -12)
    c[1::5] = (rng.integers(-4, 5, a[1::5].size) * 2.0 ** -25).astype(F)
    c[2::7] = 0
    f = libm_fmaf()
    with np.errstate(all="ignore"):
        want = np.array([f(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=F)
    got = fmaf(a, b, c)
    assert got.tobytes() == want.tobytes(), int((got.view(np.uint32) != want.view(np.uint32)).sum())


@pytest.mark.parametrize("n", [7, 15, 4099, 100003])
def test_restatement_pins_torch_cpu_adamw(n):
    """tests/adamw_restatement.py against torch.optim.AdamW(foreach=False) on CPU: six steps,
    gradients over four decades with exact zeros. exp_avg and exp_avg_sq bit-equal at every
    size and step; θ bit-equal at n <= 15 and within the project's 1e-6 normwise bound at the
    long sizes, where torch's vectorised CPU sqrt is not correctly rounded (the kernels and
    the restatement use the correctly rounded one)."""
    rng = np.random.default_rng(n)
    theta0 = rng.standard_normal(n).astype(F)
    p = torch.nn.Parameter(torch.from_numpy(theta0.copy()))
    opt = torch.optim.AdamW([p], foreach=False, **HYPER)
    st = AdamWState([theta0], **HYPER)
    for s in range(1, 7):
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 0, n)).astype(F)
        g[s % 5::5] = 0
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        st.step_grads([g])
        assert opt.state[p]["exp_avg"].numpy().tobytes() == st.m[0].tobytes(), s
        assert opt.state[p]["exp_avg_sq"].numpy().tobytes() == st.v[0].tobytes(), s
        got, want = st.theta[0], p.detach().numpy()
        err = float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())
        print(f"n={n} step {s}: theta differs in {int((got != want).sum())} elements, "
              f"normwise {err:.3g}")
        if n <= 15:
            assert got.tobytes() == want.tobytes(), s
        else:
            assert normwise_ok(got, want, 1e-6), (s, err)
    assert float(opt.state[p]["step"]) == 6.0 == float(st.t)


# ---- dispatch ------------------------------------------------------------------------------
@pytest.fixture
def oracle_backend():
    prev = kernels._DEFAULT
    k = AdamWOracleKernels()
    kernels.set_default_kernels(k)
    yield k
    kernels._DEFAULT = prev


def _models(placement):
    spec = get_tree("micro")
    shapes = [s for _, s in spec.params()]
    theta0 = synth.outer_tree(spec.numels(), spec.init_spec())
    inner = torch.nn.Module()
    inner.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(v.copy()).view(s))
                                       for v, s in zip(theta0, shapes)])
    return inner, get_outer_model(inner, placement=placement), theta0


@pytest.mark.parametrize("placement", [None, "device"])
def test_get_optimizer_dispatch_on_the_knob(placement, oracle_backend, monkeypatch):
    inner, outer, _ = _models(placement)
    monkeypatch.delenv("DILOCO_OUTER_ADAMW", raising=False)
    assert type(get_optimizer(outer, ADAMW_CFG)) is torch.optim.AdamW
    assert type(get_optimizer(inner, ADAMW_CFG)) is torch.optim.AdamW
    monkeypatch.setenv("DILOCO_OUTER_ADAMW", "torch")
    assert type(get_optimizer(outer, ADAMW_CFG)) is torch.optim.AdamW
    monkeypatch.setenv("DILOCO_OUTER_ADAMW", "fused")
    opt = get_optimizer(outer, ADAMW_CFG)
    assert type(opt) is OuterAdamW and isinstance(opt, torch.optim.AdamW)
    g = opt.param_groups[0]
    assert (g["lr"], g["betas"], g["weight_decay"], g["eps"]) == (0.01, (0.9, 0.95), 0.1, 1e-8)
    assert type(get_optimizer(inner, ADAMW_CFG)) is torch.optim.AdamW  # not an outer model
    monkeypatch.setenv("DILOCO_OUTER_ADAMW", "hip")
    with pytest.raises(ValueError, match="DILOCO_OUTER_ADAMW"):
        get_optimizer(outer, ADAMW_CFG)


def test_outer_adamw_makes_an_unrequested_exchange_replicated(oracle_backend, monkeypatch):
    """The device placement's implicit sharded default does not apply once an OuterAdamW is
    attached (the mark reaches a mirror built before or after the optimizer); an exchange that
    was asked for stays."""
    monkeypatch.delenv("DILOCO_OUTER_EXCHANGE", raising=False)
    inner, outer, _ = _models("device")
    m = outer._diloco_mirror
    assert m.exchange == "sharded" and not m.adamw_replicated
    OuterAdamW(outer, **HYPER)
    assert m.adamw_replicated and m._exchange_mode(2, False) == "replicated"
    inner, outer, _ = _models(None)  # the lazy host mirror: built at the first call
    OuterAdamW(outer, **HYPER)
    compute_pseudo_gradient(inner, outer)
    assert outer._diloco_mirror.dev.adamw_replicated
    spec = get_tree("micro")
    inner = torch.nn.Module()
    inner.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(s))
                                       for _, s in spec.params()])
    outer = get_outer_model(inner, placement="device", exchange="sharded")
    OuterAdamW(outer, **HYPER)
    assert not outer._diloco_mirror.adamw_replicated


# ---- the four calls on CPU -----------------------------------------------------------------
@pytest.fixture
def comm():
    """A one-peer TrainingComm on a process group of this test's own (destroyed afterwards:
    other tests expect none in the pytest process)."""
    from diloco_amd.comm import TrainingComm
    from diloco_amd.world import World

    made = not dist.is_initialized()
    if made:
        f = tempfile.mktemp(prefix="dl_pg_")
        dist.init_process_group("gloo", init_method=f"file://{f}", rank=0, world_size=1)
    yield TrainingComm(World.from_default_group(1), (1, 1, 32), None)
    if made:
        dist.destroy_process_group()


def _host(ts):
    return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in ts])


def _outer_step(inner, outer, opt, comm, ref, s):
    vals = synth.inner_tree(ref.theta, s, 0)
    with torch.no_grad():
        for p, v in zip(inner.parameters(), vals):
            p.copy_(torch.from_numpy(v).view(p.shape))
    compute_pseudo_gradient(inner, outer)
    comm.sync_gradients(outer)
    opt.step()
    sync_inner_model(outer, inner)
    deltas, _ = ref.step([vals])
    return deltas[0]


def _check(inner, outer, opt, ref, delta, s):
    want = np.concatenate(ref.theta).tobytes()
    assert _host(outer.parameters()).tobytes() == want, s
    assert _host(inner.parameters()).tobytes() == want, s
    assert _host(p.grad for p in outer.parameters()).tobytes() == np.concatenate(delta).tobytes(), s
    st = [opt.state[p] for p in outer.parameters()]
    assert _host(x["exp_avg"] for x in st).tobytes() == np.concatenate(ref.m).tobytes(), s
    assert _host(x["exp_avg_sq"] for x in st).tobytes() == np.concatenate(ref.v).tobytes(), s
    for x in st:
        assert x["step"].dtype == torch.float32 and x["step"].dim() == 0
        assert float(x["step"]) == float(s)


@pytest.mark.parametrize("placement", [None, "device"])
def test_four_calls_on_cpu_match_the_restatement(placement, oracle_backend, comm, monkeypatch):
    """compute_pseudo_gradient -> sync_gradients -> OuterAdamW.step -> sync_inner_model on the
    micro tree in several buckets, both placements, three steps: θ, the inner params, .grad,
    exp_avg and exp_avg_sq bit-equal to the restatement, each step ONE dl_delta_pack_adamw;
    after state_dict() -> stock AdamW.load_state_dict -> back, the next step still matches."""
    monkeypatch.setenv("DILOCO_OUTER_BUCKET_ELEMS", "4096")
    monkeypatch.setenv("DILOCO_OUTER_ADAMW", "fused")
    inner, outer, theta0 = _models(placement)
    opt = get_optimizer(outer, ADAMW_CFG)
    assert type(opt) is OuterAdamW
    ref = AdamWState(theta0, **HYPER)
    for s in (1, 2, 3):
        delta = _outer_step(inner, outer, opt, comm, ref, s)
        _check(inner, outer, opt, ref, delta, s)
    assert outer._diloco_mirror.tree.n_buckets > 2
    assert oracle_backend.calls == [("delta_pack_adamw", -1)] * 3
    # the state loads into a stock AdamW and back
    sd = opt.state_dict()
    stock = torch.optim.AdamW([torch.nn.Parameter(p.detach().cpu().clone())
                               for p in outer.parameters()], **HYPER)
    stock.load_state_dict(sd)
    for i, p in enumerate(stock.param_groups[0]["params"]):
        assert stock.state[p]["exp_avg_sq"].numpy().tobytes() == ref.v[i].tobytes()
        assert float(stock.state[p]["step"]) == 3.0
    opt.load_state_dict(stock.state_dict())
    delta = _outer_step(inner, outer, opt, comm, ref, 4)
    _check(inner, outer, opt, ref, delta, 4)
    assert oracle_backend.calls == [("delta_pack_adamw", -1)] * 4


@pytest.mark.parametrize("placement", [None, "device"])
def test_eager_mirror_steps_through_unpack_adamw(placement, oracle_backend, comm):
    """fused=False computes the delta at compute_pseudo_gradient: OuterAdamW.step is then one
    dl_unpack_adamw (divisor 1, no inner write) and sync_inner_model scatters."""
    inner, _, theta0 = _models(placement)
    outer = get_outer_model(inner, placement=placement, fused=False)
    opt = OuterAdamW(outer, **HYPER)
    ref = AdamWState(theta0, **HYPER)
    for s in (1, 2):
        delta = _outer_step(inner, outer, opt, comm, ref, s)
        _check(inner, outer, opt, ref, delta, s)
    assert oracle_backend.calls == [("unpack_adamw", -1)] * 2


# ---- fallback ------------------------------------------------------------------------------
@pytest.mark.parametrize("placement,why", [(None, "amsgrad"), ("device", "amsgrad"),
                                           (None, "beta1"), ("device", "beta1"),
                                           (None, "sync")])
def test_fallback_is_torchs_own_step(placement, why, oracle_backend):
    """Outside the kernels' contract (amsgrad; beta1 <= 0.5, where torch's lerp switches
    formula) or its mirrors (write_back="sync") OuterAdamW.step runs torch's own step body:
    three outer steps byte-equal to a stock AdamW on a plain deepcopy outer model, and neither
    AdamW kernel is launched."""
    kw = dict(HYPER)
    if why == "amsgrad":
        kw["amsgrad"] = True
    if why == "beta1":
        kw["betas"] = (0.5, 0.95)
    inner, outer, _ = _models(placement)
    if why == "sync":
        outer = get_outer_model(inner, write_back="sync")
    ref_inner = copy.deepcopy(inner)
    ref_outer = copy.deepcopy(ref_inner).to("cpu")
    opt = OuterAdamW(outer, **kw)
    ref_opt = torch.optim.AdamW(ref_outer.parameters(), **kw)
    for s in (1, 2, 3):
        prev = [p.detach().numpy().reshape(-1).copy() for p in ref_outer.parameters()]
        with torch.no_grad():
            for p, q, v in zip(inner.parameters(), ref_inner.parameters(),
                               synth.inner_tree(prev, s, 0)):
                p.copy_(torch.from_numpy(v).view(p.shape))
                q.copy_(p)
        compute_pseudo_gradient(inner, outer)
        for po, pi in zip(ref_outer.parameters(), ref_inner.parameters()):
            po.grad = po.data - pi.data
        opt.step()
        ref_opt.step()
        sync_inner_model(outer, inner)
        want = _host(ref_outer.parameters()).tobytes()
        assert _host(outer.parameters()).tobytes() == want, s
        assert _host(inner.parameters()).tobytes() == want, s
        for k in ("exp_avg", "exp_avg_sq"):
            assert _host(opt.state[p][k] for p in outer.parameters()).tobytes() == \
                _host(ref_opt.state[p][k] for p in ref_outer.parameters()).tobytes(), (s, k)
    assert not [c for c in oracle_backend.calls if "adamw" in c[0]]
