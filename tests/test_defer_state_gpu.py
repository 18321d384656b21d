"""The one-peer SGD outer step of the lazy host placement with θ and the momentum stored every
second step only (dl_delta_pack_sgd_defer / dl_delta_pack_sgd_resume, DILOCO_OUTER_DEFER_STATE):
every value a caller can observe -- θ, .grad, the momentum buffers, the inner params -- equals
the switch-off path's (one dl_delta_pack_sgd per step) bit for bit, whatever happens between
the deferred step and the one that resumes it.

The tree: tensors of 1, 3, 4, 5, 1023, 4095, 4096, 4097 and 8193 elements (tails, ragged and
several chunks) and one whose inner storage is 4-byte aligned only (the element-wise path).
The inner params get fresh non-zero noise before every step."""
import copy
import os

import numpy as np
import pytest
import torch

from diloco_amd import _lib
from diloco_amd.kernels import HipKernels
from diloco_amd.plan import SLOT_INNER
from diloco_amd.utils import (compute_pseudo_gradient, get_optimizer, get_outer_model,
                              sync_inner_model)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SIZES = [1, 3, 4, 5, 1023, 4095, 4096, 4097, 8193]
ODD = 2051  # the tensor at a 4-byte-aligned address
SWITCH = "DILOCO_OUTER_DEFER_STATE"
ALL = _lib.ALL_BUCKETS


class _Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


RULES = {"nesterov": _Cfg(type="SGD", lr=0.7, momentum=0.9, nesterov=True),
         "momentum": _Cfg(type="SGD", lr=0.7, momentum=0.9, nesterov=False),
         "plain": _Cfg(type="SGD", lr=0.7, momentum=0.0, nesterov=False)}


def _inner_model():
    g = torch.Generator().manual_seed(7)
    ps = [torch.randn(n, generator=g).to(DEV) for n in SIZES]
    base = torch.empty(ODD + 4, device=DEV)
    odd = base[1:1 + ODD]
    assert odd.data_ptr() % 16 == 4
    odd.copy_(torch.randn(ODD, generator=g))
    m = torch.nn.Module()
    m.ps = torch.nn.ParameterList([torch.nn.Parameter(t) for t in ps + [odd]])
    return m


def _noise(inner, step):
    """H inner steps' stand-in: every inner param moves by non-zero noise (the values depend
    on the step only, and nothing of the outer model is read)."""
    g = torch.Generator().manual_seed(1000 + step)
    with torch.no_grad():
        for p in inner.parameters():
            p.add_((torch.randn(p.shape, generator=g) * 1e-2 + 3e-3).to(DEV))


def _flat(ts):
    return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in ts]).copy()


class _Run:
    """The reference's outer loop (src/train.py:263-269 at one peer) on the default outer
    model, the switch on or off."""

    def __init__(self, on, rule):
        prev = os.environ.get(SWITCH)
        os.environ[SWITCH] = "1" if on else "0"
        try:
            self.inner = _inner_model()
            self.outer = get_outer_model(self.inner)
        finally:
            if prev is None:
                os.environ.pop(SWITCH)
            else:
                os.environ[SWITCH] = prev
        self.opt = get_optimizer(self.outer, RULES[rule])
        self.mirror = self.outer._diloco_mirror
        self.dev = self.mirror.dev
        assert self.dev.defer_state == on
        self.on = on
        self.steps = 0

    def step(self):
        self.steps += 1
        _noise(self.inner, self.steps)
        compute_pseudo_gradient(self.inner, self.outer)
        self.opt.step()
        sync_inner_model(self.outer, self.inner)

    def pending(self):
        return self.dev._pend is not None

    def read(self):
        """What a caller can observe, as bytes: inner, .grad (neither completes a pending
        step), the momentum buffers, θ."""
        ps = list(self.outer.parameters())
        out = {"inner": _flat(self.inner.parameters()), "grad": _flat(p.grad for p in ps)}
        if "momentum_buffer" in self.opt.state.get(ps[0], {}):
            out["momentum"] = _flat(self.opt.state[p]["momentum_buffer"] for p in ps)
        out["theta"] = _flat(ps)
        assert not self.pending()
        return {k: v.tobytes() for k, v in out.items()}

    def close(self):
        self.mirror.close()


_REF = {}


def _reference(rule):
    """The switch-off path, read after each of 5 steps (computed once per rule; reading
    changes nothing there: every step stores all it computes)."""
    if rule not in _REF:
        r = _Run(False, rule)
        _REF[rule] = []
        for _ in range(5):
            r.step()
            _REF[rule].append(r.read())
        r.close()
    return _REF[rule]


@pytest.mark.parametrize("rule", list(RULES))
def test_read_after_every_step(rule):
    """A read after every step: every deferred step is completed by dl_unpack_sgd (the first
    one with the first-step rule), never resumed."""
    ref = _reference(rule)
    r = _Run(True, rule)
    for s in range(5):
        r.step()
        assert r.pending()
        assert r.read() == ref[s], (rule, s + 1)
    r.close()


@pytest.mark.parametrize("steps", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("rule", list(RULES))
def test_read_after_the_last_step_only(rule, steps):
    """Nothing read in between: defer, resume, defer, ... (the first step's first-step rule
    is the pending one of step 2); an odd count ends with a step pending."""
    ref = _reference(rule)
    r = _Run(True, rule)
    for s in range(steps):
        r.step()
        assert r.pending() == (s % 2 == 0)
    assert r.read() == ref[steps - 1]
    r.close()


@pytest.mark.parametrize("at", [2, 3])
def test_hyperparameters_changed_between_steps(at):
    """lr and momentum changed before step `at`: 2 = between a deferred step and the one that
    resumes it (the kernel gets both sets), 3 = between a resumed and a deferred one."""
    def run(on):
        r = _Run(on, "nesterov")
        for s in range(1, 5):
            if s == at:
                r.opt.param_groups[0]["lr"] = 0.35
                r.opt.param_groups[0]["momentum"] = 0.8
            r.step()
            assert not on or r.pending() == (s % 2 == 1)
        out = r.read()
        r.close()
        return out

    assert run(True) == run(False)


def _ev_read_param(r, box):
    box["seen"] = next(r.outer.parameters()).detach().clone().numpy().tobytes()


def _ev_write_theta(r, box):
    with torch.no_grad():
        list(r.outer.parameters())[4].add_(0.25)


def _ev_write_grad(r, box):
    with torch.no_grad():
        list(r.outer.parameters())[5].grad.add_(1.0)


def _ev_load_state_dict(r, box):
    r.opt.load_state_dict(box["sd"])  # plain tensors: nothing of the outer model is read


def _ev_realloc_inner(r, box):
    for p in r.inner.parameters():
        p.data = p.data.clone()


def _ev_zero_grad_none(r, box):
    r.opt.zero_grad(set_to_none=True)


def _ev_zero_grad_zero(r, box):
    r.opt.zero_grad(set_to_none=False)


def _ev_deepcopy(r, box):
    c = copy.deepcopy(r.outer)
    assert all(type(p) is torch.nn.Parameter for p in c.parameters())
    box["seen"] = _flat(c.parameters()).tobytes()


EVENTS = {"read_param": _ev_read_param, "write_theta": _ev_write_theta,
          "write_grad": _ev_write_grad, "load_state_dict": _ev_load_state_dict,
          "realloc_inner": _ev_realloc_inner, "zero_grad_none": _ev_zero_grad_none,
          "zero_grad_zero": _ev_zero_grad_zero, "deepcopy": _ev_deepcopy}


@pytest.mark.parametrize("event", list(EVENTS))
def test_event_while_a_step_is_pending(event):
    """Step 1 read (so the optimizer's state_dict exists), step 2 deferred, the event with
    that step pending, two more steps, everything read: the same bytes as with the switch
    off, and whatever the event itself saw."""
    def run(on):
        r = _Run(on, "nesterov")
        box = {}
        r.step()
        first = r.read()
        box["sd"] = copy.deepcopy(r.opt.state_dict())  # the state after step 1, momentum halved
        for st in box["sd"]["state"].values():
            st["momentum_buffer"].mul_(0.5)
        r.step()
        assert r.pending() == on
        EVENTS[event](r, box)
        r.step()
        r.step()
        out = (first, box.get("seen"), r.read())
        r.close()
        return out

    assert run(True) == run(False)


def test_close_with_a_step_pending():
    """close() completes the pending step: the host tensors hold the step afterwards (nothing
    can continue on a closed mirror)."""
    ref = _reference("nesterov")
    r = _Run(True, "nesterov")
    r.step()
    assert r.pending()
    r.close()
    assert not r.pending()
    assert r.read() == ref[0]


# ---- the kernels on raw buffers ------------------------------------------------------------
class _Raw:
    """A tree of the test's tensors with packed θ, momentum and wire arenas, and inner params
    of its own; `flags`: the store policy (both are instantiated in the product library)."""

    def __init__(self, flags):
        self.k = HipKernels()
        self.inner = [p.detach() for p in _inner_model().parameters()]
        numels = [p.numel() for p in self.inner]
        self.tree = self.k.tree(numels, DEV)
        self.tree.tune(0, flags)
        z = dict(dtype=torch.float32, device=DEV)
        self.theta = torch.zeros(self.tree.total, **z)
        self.mom = torch.full((self.tree.total,), 7.0, **z)  # never read before it is written
        self.wire = torch.full((self.tree.total,), -3.0, **z)
        g = torch.Generator().manual_seed(11)
        for o, n in zip(self.tree.seg_off[:-1], numels):
            self.theta[int(o):int(o) + n].copy_(torch.randn(n, generator=g))
        self.k.bind(self.tree, SLOT_INNER, self.inner, DEV)

    def noise(self, step):
        g = torch.Generator().manual_seed(2000 + step)
        for p in self.inner:
            p.add_((torch.randn(p.shape, generator=g) * 1e-2 + 3e-3).to(DEV))

    def state(self, momentum):
        torch.cuda.synchronize()
        out = [self.theta, self.wire] + ([self.mom] if momentum else []) + self.inner
        return [t.cpu().numpy().tobytes() for t in out]


HYPER = {"nesterov": ((0.7, 0.9, True), (0.35, 0.8, True)),
         "momentum": ((0.7, 0.9, False), (0.7, 0.9, False)),
         "plain": ((0.7, 0.0, False), (0.35, 0.0, False)),
         "momentum_off": ((0.7, 0.9, True), (0.7, 0.0, False)),
         "momentum_on": ((0.7, 0.0, False), (0.7, 0.9, True))}


@pytest.mark.parametrize("flags", [_lib.TUNE_NT_LOADS, _lib.TUNE_NT_LOADS | _lib.TUNE_NT_STORES])
@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("rule", list(HYPER))
def test_defer_then_resume_equals_two_steps(rule, first, flags):
    """dl_delta_pack_sgd_defer then dl_delta_pack_sgd_resume = dl_delta_pack_sgd twice, and
    defer then dl_unpack_sgd (divisor 1, no inner write) = dl_delta_pack_sgd once: θ, the wire,
    the momentum and inner, for every pair of SGD modes (first: the deferred step is the first
    one) and independent hyper-parameters of the two steps."""
    (lr1, m1, n1), (lr2, m2, n2) = HYPER[rule]
    a, b, c = _Raw(flags), _Raw(flags), _Raw(flags)
    if not first:  # a step before, so the momentum holds values
        for r in (a, b, c):
            r.noise(0)
            r.k.delta_pack_sgd(r.tree, ALL, SLOT_INNER, r.theta, r.wire, r.mom if m1 else None,
                               lr1, m1, n1, True)
    # a momentum switched on at the second step starts from the buffer's first-step rule
    first2 = m2 != 0 and m1 == 0
    for r in (a, b, c):
        r.noise(1)
    theta0, mom0 = a.theta.clone(), a.mom.clone()
    a.k.delta_pack_sgd(a.tree, ALL, SLOT_INNER, a.theta, a.wire, a.mom if m1 else None, lr1, m1,
                       n1, first)
    for r in (b, c):
        r.k.delta_pack_sgd_defer(r.tree, ALL, SLOT_INNER, r.theta, r.wire, r.mom if m1 else None,
                                 lr1, m1, n1, first)
    torch.cuda.synchronize()
    # the deferred step: wire and inner as the full step's, θ and the momentum untouched
    assert torch.equal(b.wire.view(torch.int32), a.wire.view(torch.int32))
    for p, q in zip(b.inner, a.inner):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32))
    assert torch.equal(b.theta.view(torch.int32), theta0.view(torch.int32))
    assert torch.equal(b.mom.view(torch.int32), mom0.view(torch.int32))
    # settled: the full step
    c.k.unpack_sgd(c.tree, ALL, c.wire, 1, c.theta, c.mom if m1 else None, lr1, m1, n1, first, -1)
    assert c.state(m1) == a.state(m1)
    # resumed: two full steps
    for r in (a, b):
        r.noise(2)
    a.k.delta_pack_sgd(a.tree, ALL, SLOT_INNER, a.theta, a.wire, a.mom if m2 else None, lr2, m2,
                       n2, first2)
    b.k.delta_pack_sgd_resume(b.tree, ALL, SLOT_INNER, b.theta, b.wire,
                              b.mom if (m1 or m2) else None, (lr1, m1, n1, first), lr2, m2, n2,
                              first2)
    assert b.state(m1 or m2) == a.state(m1 or m2)
    for r in (a, b, c):
        r.tree.close()
