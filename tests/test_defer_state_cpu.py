"""The pending-step bookkeeping of the lazy host placement's one-peer SGD step (θ and the
momentum stored every second step only, DILOCO_OUTER_DEFER_STATE) on the CPU, through the
oracle kernel backend extended with the defer / resume pair: which kernel each step runs, what
completes a pending step and what does not, and the reference's values whatever was read. The
kernels themselves are tests/test_defer_state_gpu.py."""
import copy

import numpy as np
import pytest
import torch

from conftest import load_npz
from diloco_amd import kernels, synth
from diloco_amd.trees import get_tree
from diloco_amd.utils import (compute_pseudo_gradient, get_optimizer, get_outer_model,
                              sync_inner_model)
from oracle_kernels import OracleKernels


class _Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


SGD_CFG = _Cfg(type="SGD", lr=0.7, momentum=0.9, nesterov=True)


class _DeferKernels(OracleKernels):
    """The checker backend with the defer / resume pair restated from its own kernels, and a
    log of the outer-step launches the mirror makes."""

    def __init__(self):
        self.log = []
        self._depth = 0

    def _logged(self, name, f, *a):
        if self._depth == 0:
            self.log.append(name)
        self._depth += 1
        try:
            return f(*a)
        finally:
            self._depth -= 1

    def delta_pack(self, *a):
        return self._logged("delta_pack", super().delta_pack, *a)

    def unpack_sgd(self, *a):
        return self._logged("unpack_sgd", super().unpack_sgd, *a)

    def delta_pack_sgd(self, *a):
        return self._logged("delta_pack_sgd", super().delta_pack_sgd, *a)

    def scatter(self, *a):
        return self._logged("scatter", super().scatter, *a)

    def delta_pack_sgd_defer(self, tree, bucket, inner_slot, theta, wire, mom, lr, momentum,
                             nesterov, first):
        def run():  # the full step on copies of θ and the momentum: only wire and inner land
            th, b = theta.clone(), None if mom is None else mom.clone()
            self.delta_pack_sgd(tree, bucket, inner_slot, th, wire, b, lr, momentum, nesterov,
                                first)
        return self._logged("defer", run)

    def delta_pack_sgd_resume(self, tree, bucket, inner_slot, theta, wire, mom, pending, lr,
                              momentum, nesterov, first):
        def run():
            p_lr, p_momentum, p_nesterov, p_first = pending
            self.unpack_sgd(tree, bucket, wire, 1, theta, mom if p_momentum else None, p_lr,
                            p_momentum, p_nesterov, p_first, -1)
            self.delta_pack_sgd(tree, bucket, inner_slot, theta, wire, mom if momentum else None,
                                lr, momentum, nesterov, first)
        return self._logged("resume", run)


@pytest.fixture()
def k():
    prev = kernels._DEFAULT
    k = _DeferKernels()
    kernels.set_default_kernels(k)
    yield k
    kernels._DEFAULT = prev


def _models():
    spec = get_tree("micro")
    shapes = [s for _, s in spec.params()]
    theta0 = synth.outer_tree(spec.numels(), spec.init_spec())
    inner = torch.nn.Module()
    inner.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(v.copy()).view(s))
                                       for v, s in zip(theta0, shapes)])
    return inner, get_outer_model(inner)


def _host(ts):
    return np.concatenate([t.detach().numpy().reshape(-1) for t in ts])


def _step(inner, outer, opt, prev, s):
    """Outer step s of the fixture: inner = θ_{s-1} + the fixture's noise (prev: θ_{s-1} from
    the fixture, so nothing of the outer model is read)."""
    numels = [p.numel() for p in inner.parameters()]
    theta = np.split(prev, np.cumsum(numels)[:-1])
    with torch.no_grad():
        for p, v in zip(inner.parameters(), synth.inner_tree(theta, s, 0)):
            p.copy_(torch.from_numpy(v).view(p.shape))
    compute_pseudo_gradient(inner, outer)
    opt.step()
    sync_inner_model(outer, inner)


def test_switch_is_read_when_the_mirror_is_built(k, monkeypatch):
    _, outer = _models()
    assert outer._diloco_mirror.dev.defer_state
    monkeypatch.setenv("DILOCO_OUTER_DEFER_STATE", "0")
    _, outer = _models()
    assert not outer._diloco_mirror.dev.defer_state
    # a kernel set without the pair, and every other way to the fused step, keep one kernel
    kernels.set_default_kernels(OracleKernels())
    monkeypatch.delenv("DILOCO_OUTER_DEFER_STATE")
    _, outer = _models()
    assert not outer._diloco_mirror.dev.defer_state
    kernels.set_default_kernels(k)
    inner = _models()[0]
    assert not get_outer_model(inner, wire="bf16")._diloco_mirror.dev.defer_state
    assert not get_outer_model(inner, fused=False)._diloco_mirror.dev.defer_state
    assert not get_outer_model(inner, placement="device")._diloco_mirror.defer_state


def test_steps_alternate_and_reads_complete_a_pending_step(k):
    g = load_npz("micro_n1.npz")
    inner, outer = _models()
    m = outer._diloco_mirror
    opt = get_optimizer(outer, SGD_CFG)
    ps = list(outer.parameters())
    _step(inner, outer, opt, g["theta0"], 1)
    assert k.log == ["defer"] and m.dev._pend == (0.7, 0.9, True, True)
    # inner and .grad are the step's already; reading them completes nothing
    assert _host(inner.parameters()).tobytes() == g["theta_s1"].tobytes()
    assert _host(p.grad for p in ps).tobytes() == g["delta_s1_r0"].tobytes()
    assert k.log == ["defer"] and m.dev._pend is not None
    _step(inner, outer, opt, g["theta_s1"], 2)
    assert k.log == ["defer", "resume"] and m.dev._pend is None
    assert _host(ps).tobytes() == g["theta_s2"].tobytes()
    assert _host(opt.state[p]["momentum_buffer"] for p in ps).tobytes() == g["buf_s2"].tobytes()
    assert _host(p.grad for p in ps).tobytes() == g["delta_s2_r0"].tobytes()
    assert _host(inner.parameters()).tobytes() == g["theta_s2"].tobytes()
    assert k.log == ["defer", "resume"]  # nothing was pending: the reads ran no kernel


@pytest.mark.parametrize("read", ["theta", "momentum", "state_dict", "opt_state_dict",
                                  "deepcopy", "write_theta", "write_grad", "close"])
def test_what_completes_a_pending_step(k, read):
    g = load_npz("micro_n1.npz")
    inner, outer = _models()
    m = outer._diloco_mirror
    opt = get_optimizer(outer, SGD_CFG)
    ps = list(outer.parameters())
    _step(inner, outer, opt, g["theta0"], 1)
    assert k.log == ["defer"]
    theta = None
    if read == "theta":
        theta = ps[0].detach().clone()
    elif read == "momentum":
        assert _host(opt.state[p]["momentum_buffer"]
                     for p in ps).tobytes() == g["buf_s1"].tobytes()
    elif read == "state_dict":
        assert _host(outer.state_dict().values()).tobytes() == g["theta_s1"].tobytes()
    elif read == "opt_state_dict":
        sd = opt.state_dict()["state"]
        assert _host(sd[i]["momentum_buffer"]
                     for i in range(len(sd))).tobytes() == g["buf_s1"].tobytes()
    elif read == "deepcopy":
        assert _host(copy.deepcopy(outer).parameters()).tobytes() == g["theta_s1"].tobytes()
    elif read == "write_theta":
        with torch.no_grad():
            ps[0].add_(0.0)
    elif read == "write_grad":
        with torch.no_grad():
            ps[0].grad.add_(0.0)
        assert k.log == ["defer"]  # reading .grad: nothing; the upload comes with the next call
        compute_pseudo_gradient(inner, outer)
    elif read == "close":
        m.close()
    assert k.log == ["defer", "unpack_sgd"] and m.dev._pend is None
    assert theta is None or theta.numpy().tobytes() == _host(ps[:1]).tobytes()
    assert _host(ps).tobytes() == g["theta_s1"].tobytes()
    assert _host(opt.state[p]["momentum_buffer"] for p in ps).tobytes() == g["buf_s1"].tobytes()
    if read == "close":
        return
    # the next step starts the cycle again, and is the reference's
    _step(inner, outer, opt, g["theta_s1"], 2)
    assert k.log[-1] == "defer" and "resume" not in k.log
    assert _host(ps).tobytes() == g["theta_s2"].tobytes()
    assert _host(opt.state[p]["momentum_buffer"] for p in ps).tobytes() == g["buf_s2"].tobytes()
    assert _host(p.grad for p in ps).tobytes() == g["delta_s2_r0"].tobytes()


def test_hyperparameters_of_the_pending_step_are_kept(k):
    """lr and momentum changed while a step is pending: the resume gets that step's own
    scalars, and so does a settle."""
    g = load_npz("micro_n1.npz")
    inner, outer = _models()
    m = outer._diloco_mirror
    opt = get_optimizer(outer, SGD_CFG)
    _step(inner, outer, opt, g["theta0"], 1)
    opt.param_groups[0]["lr"] = 0.1
    opt.param_groups[0]["momentum"] = 0.5
    assert m.dev._pend == (0.7, 0.9, True, True)
    assert _host(outer.parameters()).tobytes() == g["theta_s1"].tobytes()
    assert k.log == ["defer", "unpack_sgd"]
