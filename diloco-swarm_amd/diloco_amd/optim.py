"""The outer optimizer: torch.optim.SGD's interface, the HIP fused update underneath.

`get_optimizer(outer_model, cfg)` with cfg.type == "SGD" (src/utils.py:62-63; the DiLoCo
runs use Nesterov, configs/optimizer/nesterov.toml, lr 0.7 at experiments/experiment1.sh:65)
returns an `OuterSGD`. It IS a torch.optim.SGD (param_groups, state_dict, LR schedulers work
unchanged) whose step() runs `_single_tensor_sgd`'s arithmetic for the whole tree in one
dl_unpack_sgd launch on the device mirror of the outer model (mirror.HostOuterMirror), then
writes θ and the momentum buffers back to the host tensors the optimizer owns; on the device
outer model (mirror.DeviceOuterMirror) its state's momentum buffers are views of the packed
HBM momentum (mirror.MomentumBuffer).

With cfg.type == "AdamW" (src/utils.py:60-61) and DILOCO_OUTER_ADAMW=fused it returns an
`OuterAdamW`: torch.optim.AdamW's interface over dl_delta_pack_adamw / dl_unpack_adamw, and
over dl_shard_adamw / dl_shard_reduce_adamw under the sharded and rank-order exchanges.

The INNER optimizer (src/train.py:257, stepped every training step) is stock torch.optim.AdamW
unless DILOCO_INNER_ADAMW=fused: then get_optimizer returns an `InnerAdamW` for a model that is
not an outer model, whose step is one dl_adamw_step pass over the model's own tensors
(28 B/param where torch's foreach step makes nine passes).
"""
from __future__ import annotations

import inspect
from operator import is_, methodcaller

import torch
from torch.optim import SGD, AdamW

from ._lib import ALL_BUCKETS
from .kernels import adamw_scalars, default_kernels
from .mirror import HostOuterMirror
from .plan import SLOT_GRAD, SLOT_INNER

_MOMENTUM_BUFFER = methodcaller("get", "momentum_buffer")
_ADAM_KEYS = ("step", "exp_avg", "exp_avg_sq")


class OuterSGD(SGD):
    def __init__(self, model: torch.nn.Module, lr: float, momentum: float = 0.0,
                 nesterov: bool = False):
        super().__init__(model.parameters(), lr=lr, momentum=momentum, nesterov=nesterov)
        self._model = model

    def _mirror(self) -> HostOuterMirror:
        from .utils import outer_mirror  # local import: utils builds on this module

        return outer_mirror(self._model)

    def state_dict(self):
        """torch.optim.SGD.state_dict, after a deferred write-back of the momentum landed."""
        from .utils import flush_outer_model

        flush_outer_model(self._model)
        return super().state_dict()

    @torch.no_grad()
    def step(self, closure=None):
        """One outer SGD step (src/train.py:267). torch.optim.Optimizer wraps it as it wraps
        every optimizer's step (its profiler annotation, the global and per-optimizer pre /
        post hooks), so hooks and LR schedulers see an ordinary SGD."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if len(self.param_groups) != 1:
            raise NotImplementedError("OuterSGD: one parameter group (as get_optimizer builds)")
        g = self.param_groups[0]
        if g["weight_decay"] != 0 or g["dampening"] != 0 or g["maximize"]:
            raise NotImplementedError(
                "OuterSGD implements SGD as src/utils.py:63 builds it: weight_decay=0, "
                "dampening=0, maximize=False")
        if g["nesterov"] and g["momentum"] == 0:
            raise ValueError("Nesterov momentum requires a momentum")
        mirror = getattr(self._model, "_diloco_mirror", None)  # utils._ATTR
        if mirror is None:
            from .utils import device_path
        if mirror is None and not device_path(g["params"][0]):
            # host tensors never stepped on the GPU (the reference's --device cpu runs):
            # torch.optim.SGD's own step body, as src/utils.py:62-63 builds it -- unwrapped,
            # since this call already runs inside the hook wrapper (no_grad is ours)
            inspect.unwrap(SGD.step)(self)
            return loss
        if mirror is None:
            mirror = self._mirror()
        params = g["params"]
        if len(params) != len(mirror.params) or not all(map(is_, params, mirror.params)):
            raise RuntimeError("OuterSGD parameters differ from its model's parameters()")
        momentum = float(g["momentum"])
        # self.state is keyed by tensor (a Python __hash__ per lookup): when it holds exactly
        # the parameters in order -- every step after the first -- walk its values instead
        st = self.state
        same = len(st) == len(params) and all(map(is_, st.keys(), params))
        if same:
            host_bufs = list(map(_MOMENTUM_BUFFER, st.values()))
        else:
            host_bufs = [st[p].get("momentum_buffer") for p in params]
        lr = g["lr"]
        if isinstance(lr, torch.Tensor):
            lr = float(lr.item())
        bufs = mirror.sgd_step(float(lr), momentum, bool(g["nesterov"]), host_bufs)
        if momentum != 0:
            if same and all(map(is_, host_bufs, bufs)):
                pass  # the state already holds these buffers (every step after the first)
            elif same:
                for v, b in zip(st.values(), bufs):
                    v["momentum_buffer"] = b
            else:
                for p, b in zip(params, bufs):
                    st[p]["momentum_buffer"] = b
        return loss


class OuterAdamW(AdamW):
    """The AdamW outer optimizer (src/utils.py:60-61, configs/optimizer/adamw.toml) with its
    step fused into the outer model's mirror: at one peer the whole outer step is one
    dl_delta_pack_adamw pass (36 B/param), at N > 1 one dl_unpack_adamw pass per bucket after
    the replicated exchange; after the sharded exchange (asked for: exchange="sharded") one
    dl_shard_adamw per bucket on this rank's 1/n, after the rank-order one
    (DILOCO_DP_EXCHANGE=a2a, bit-exact at every replica count) one dl_shard_reduce_adamw, each
    followed by the all_gather of θ; after the int8 exchange (wire="int8") one
    dl_unpack_adamw_q8 per bucket on the averaged slots, the whole tree on every rank (the fp4
    exchange, wire="fp4": dl_unpack_adamw_fp4 in its place). It IS a torch.optim.AdamW (param_groups, hooks, LR
    schedulers and state_dict work unchanged; state[p]["step"] is torch's fp32 scalar tensor,
    exp_avg and exp_avg_sq are views of the mirror's packed arenas), selected by get_optimizer
    under DILOCO_OUTER_ADAMW=fused. After a sharded or rank-order step each rank holds its own
    1/n of exp_avg and exp_avg_sq; reading either, or state_dict(), gathers the rest first -- a
    collective over the DP group, like reading the momentum of a sharded OuterSGD.

    The fused pass is one element of torch's _single_tensor_adamw (include/diloco_hip.h).
    Whenever that contract or the mirror does not cover the step -- amsgrad, maximize,
    capturable, differentiable, beta1 <= 0.5, tensor hyper-parameters, more than one group,
    parameters whose step counts differ, write_back "sync" or "deferred", no mirror at all (a CPU-only run) -- step() runs torch's own step body, exactly
    what a stock AdamW on this outer model does: never a silently different result."""

    def __init__(self, model: torch.nn.Module, lr: float = 1e-3, betas=(0.9, 0.999),
                 weight_decay: float = 1e-2, eps: float = 1e-8, **kw):
        super().__init__(model.parameters(), lr=lr, betas=betas, eps=eps,
                         weight_decay=weight_decay, **kw)
        self._model = model
        from .utils import mark_adamw_outer

        mark_adamw_outer(model)  # an unrequested exchange becomes the replicated one

    def state_dict(self):
        """torch.optim.AdamW.state_dict, after the mirror's pending work landed."""
        from .utils import flush_outer_model

        flush_outer_model(self._model)
        return super().state_dict()

    def _fused_plan(self):
        """(mirror, scalars of this step, exp_avg list, exp_avg_sq list, states) when the
        fused pass computes exactly what torch's step body would; else None."""
        if len(self.param_groups) != 1:
            return None
        g = self.param_groups[0]
        if (g["amsgrad"] or g["maximize"] or g.get("capturable") or g.get("differentiable")
                or g.get("fused") or not g.get("decoupled_weight_decay", True)):
            return None
        hyper = (g["lr"], g["betas"][0], g["betas"][1], g["weight_decay"], g["eps"])
        if any(isinstance(x, torch.Tensor) for x in hyper):
            return None
        lr, beta1, beta2, wd, eps = map(float, hyper)
        if not beta1 > 0.5:  # torch's lerp switches formula at weight 0.5
            return None
        mirror = getattr(self._model, "_diloco_mirror", None)  # utils._ATTR
        if mirror is None or not hasattr(mirror, "adamw_step") or not mirror.adamw_ready():
            return None
        params = g["params"]
        if len(params) != len(mirror.params) or not all(map(is_, params, mirror.params)):
            return None
        states = [self.state[p] for p in params]
        have = [len(s) != 0 for s in states]
        if any(have) and not all(have):
            return None
        step = 0.0
        if have[0]:
            if any(set(s) != set(_ADAM_KEYS) for s in states):
                return None
            steps = [s["step"] for s in states]
            if any(t.device.type != "cpu" for t in steps):
                return None
            step = float(steps[0])
            if any(float(t) != step for t in steps):
                return None
        scalars = adamw_scalars(lr, beta1, beta2, wd, eps, step + 1.0)
        return (mirror, scalars, [s.get("exp_avg") for s in states],
                [s.get("exp_avg_sq") for s in states], states)

    @torch.no_grad()
    def step(self, closure=None):
        """One outer AdamW step (src/train.py:267), wrapped by torch.optim.Optimizer like every
        optimizer's step (profiler annotation, pre / post hooks)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        plan = self._fused_plan()
        if plan is None:
            # torch's own step body, unwrapped: this call already runs inside the hook wrapper
            inspect.unwrap(AdamW.step)(self)
            return loss
        mirror, scalars, host_m, host_v, states = plan
        ms, vs = mirror.adamw_step(scalars, host_m, host_v)
        if not states[0]:
            from torch.optim.optimizer import _get_scalar_dtype

            for s in states:
                s["step"] = torch.tensor(0.0, dtype=_get_scalar_dtype())
        torch._foreach_add_([s["step"] for s in states], 1)
        if not all(map(is_, host_m, ms)) or not all(map(is_, host_v, vs)):
            for s, m, v in zip(states, ms, vs):
                s["exp_avg"], s["exp_avg_sq"] = m, v
        return loss


_NONFINITE = ("The total norm of order 2.0 for gradients from `parameters` is non-finite, so it "
              "cannot be clipped. To disable this error and scale the gradients by the "
              "non-finite norm anyway, set `error_if_nonfinite=False`")


class InnerAdamW(AdamW):
    """The inner optimizer (src/utils.py:60-61 on the inner model, stepped at src/train.py:257)
    with its step fused into ONE dl_adamw_step pass over the model's own tensors: g, θ, exp_avg
    and exp_avg_sq read once, θ, exp_avg and exp_avg_sq written once (28 B/param), where
    torch's _multi_tensor_adam makes nine foreach passes. Same constructor as
    torch.optim.AdamW, and it IS one: param_groups, hooks, LR schedulers, state_dict and
    load_state_dict work unchanged and interoperate with stock AdamW in both directions
    (state[p]["step"] is torch's CPU fp32 scalar tensor; exp_avg and exp_avg_sq are views,
    shaped like p, of two packed fp32 arenas this optimizer owns). Selected by get_optimizer
    under DILOCO_INNER_ADAMW=fused.

    Nothing is built on the device before the first fused step (the reference makes the
    optimizer while the model is still on the CPU and moves the model afterwards): that step
    builds a PackedTree over the group's numels on the parameters' device and the two zero
    arenas. Every fused step binds the parameters and this step's .grad tensors (keyed by
    address: no work while they are unchanged, no host stall when they are not), computes the
    seven scalars from the group's current lr, launches once over the whole tree and adds 1
    to the step counts on the host. It never synchronises with the device.

    The fused pass is one element of torch's _single_tensor_adamw (include/diloco_hip.h). It is
    taken only when it computes exactly that: one param group; no amsgrad, maximize,
    capturable, differentiable or fused; decoupled weight decay; float hyper-parameters;
    beta1 > 0.5; every parameter fp32, contiguous and on one device that takes the HIP path,
    each with a dense, contiguous fp32 .grad there; the state empty for all parameters or
    complete for all with equal step counts in CPU tensors. In every other case step() runs
    torch's own step body, in place on the arena views where they exist: never a silently
    different result. A fallback that leaves the step counts unequal (a parameter without a
    .grad for one step) makes the fallback permanent. State that is not the arena views --
    after load_state_dict, or created by a fallback -- is copied into the arenas and the views
    are installed again before the next fused step."""

    # Device-side pieces, built by the first fused step. Class-level defaults: torch pickles an
    # optimizer as (defaults, state, param_groups) only, so a copy starts without them.
    _tree = None      # the optimizer's own tree: not the clip cache's (LRU-closed)
    _tree_key = None  # (backend, device, numels) it was built for
    _m = _v = None    # the packed exp_avg / exp_avg_sq arenas
    _m_views = _v_views = ()
    _partials = None
    _pending = None   # (out2, gradient addresses, the gradients) of clip_grad_norm_

    def _fused_plan(self):
        """(kernels, device, params, grads, scalars of this step, states) when the fused pass
        computes exactly what torch's step body would; else None."""
        if len(self.param_groups) != 1:
            return None
        g = self.param_groups[0]
        if (g["amsgrad"] or g["maximize"] or g.get("capturable") or g.get("differentiable")
                or g.get("fused") or not g.get("decoupled_weight_decay", True)):
            return None
        hyper = (g["lr"], g["betas"][0], g["betas"][1], g["weight_decay"], g["eps"])
        if any(isinstance(x, torch.Tensor) for x in hyper):
            return None
        lr, beta1, beta2, wd, eps = map(float, hyper)
        if not beta1 > 0.5:  # torch's lerp switches formula at weight 0.5
            return None
        params = g["params"]
        if not params:
            return None
        from .utils import device_path  # local import: utils builds on this module

        dev = params[0].device
        if not device_path(params[0]):
            return None
        grads = []
        for p in params:
            gr = p.grad
            if (gr is None or p.dtype != torch.float32 or gr.dtype != torch.float32
                    or p.device != dev or gr.device != dev or gr.layout != torch.strided
                    or not p.is_contiguous() or not gr.is_contiguous()):
                return None
            grads.append(gr)
        states = [self.state.get(p) or None for p in params]
        have = [s is not None for s in states]
        if any(have) and not all(have):
            return None
        step = 0.0
        if have[0]:
            if any(set(s) != set(_ADAM_KEYS) for s in states):
                return None
            steps = [s["step"] for s in states]
            if any(not isinstance(t, torch.Tensor) or t.device.type != "cpu" for t in steps):
                return None
            step = float(steps[0])
            if any(float(t) != step for t in steps):
                return None
            if any(s["exp_avg"].shape != p.shape or s["exp_avg_sq"].shape != p.shape
                   for s, p in zip(states, params)):
                return None
        else:
            states = None
        scalars = adamw_scalars(lr, beta1, beta2, wd, eps, step + 1.0)
        return default_kernels(), dev, params, grads, scalars, states

    def _ensure_arenas(self, k, dev, params, states):
        """The tree and the arenas for these parameters (built on first use, or again when the
        parameters moved), with state[p] holding the arena views; returns the states."""
        key = (k.name, dev, tuple(p.numel() for p in params))
        if self._tree is None or self._tree_key != key:
            if self._tree is not None:
                self._tree.close()
            self._tree = tree = k.tree(key[2], dev)
            self._tree_key = key
            self._m = torch.zeros(tree.total, dtype=torch.float32, device=dev)
            self._v = torch.zeros(tree.total, dtype=torch.float32, device=dev)
            offs = [int(o) for o in tree.seg_off[:-1]]
            self._m_views = [self._m[o:o + p.numel()].view(p.shape) for o, p in zip(offs, params)]
            self._v_views = [self._v[o:o + p.numel()].view(p.shape) for o, p in zip(offs, params)]
            self._partials = None
        elif states is None:  # the state was dropped: the arenas start from zero again
            self._m.zero_()
            self._v.zero_()
        if states is None:
            from torch.optim.optimizer import _get_scalar_dtype

            states = []
            for p, m, v in zip(params, self._m_views, self._v_views):
                s = self.state[p]
                s["step"] = torch.tensor(0.0, dtype=_get_scalar_dtype())
                s["exp_avg"], s["exp_avg_sq"] = m, v
                states.append(s)
            return states
        for s, m, v in zip(states, self._m_views, self._v_views):
            if s["exp_avg"] is not m:  # loaded, or created by torch's step body: adopt
                m.copy_(s["exp_avg"])
                s["exp_avg"] = m
            if s["exp_avg_sq"] is not v:
                v.copy_(s["exp_avg_sq"])
                s["exp_avg_sq"] = v
        return states

    def _bind(self, k, dev, params, grads):
        pkey = tuple([p.data_ptr() for p in params])
        gkey = tuple([gr.data_ptr() for gr in grads])
        k.bind(self._tree, SLOT_INNER, params, dev, key=pkey)
        k.bind(self._tree, SLOT_GRAD, grads, dev, key=gkey)  # .grad is reallocated every step
        return gkey

    @torch.no_grad()
    def clip_grad_norm_(self, max_norm: float, error_if_nonfinite: bool = False) -> torch.Tensor:
        """The 2-norm of the group's gradients, as utils.clip_grad_norm_ computes it
        (dl_grad_sumsq -> dl_norm_finish on this optimizer's own tree; the same bits), with
        the clipping folded into the next step(): the clip coefficient stays on the device and
        step() hands it to dl_adamw_step, which multiplies each gradient by it as it reads it.

        Unlike torch.nn.utils.clip_grad_norm_ this leaves the gradients UNSCALED: .grad holds
        the raw values before and after step(); only the update sees them clipped (θ, exp_avg
        and exp_avg_sq equal utils.clip_grad_norm_ followed by step() bit for bit). The
        coefficient belongs to the gradient tensors it was computed from: a step() that finds
        other gradient tensors, or that cannot take the fused pass, raises RuntimeError;
        zero_grad() drops it. When the fused pass does not apply now, this call is
        utils.clip_grad_norm_ on the parameters (gradients scaled in place, nothing pending)."""
        self._pending = None
        plan = self._fused_plan()
        if plan is None:
            from .utils import clip_grad_norm_

            params = [p for g in self.param_groups for p in g["params"]]
            return clip_grad_norm_(params, max_norm, error_if_nonfinite=error_if_nonfinite)
        k, dev, params, grads, _, states = plan
        self._ensure_arenas(k, dev, params, states)
        tree = self._tree
        if self._partials is None:
            self._partials = torch.zeros(max(1, tree.n_chunks), dtype=torch.float64, device=dev)
        out2 = torch.empty(2, dtype=torch.float32, device=dev)  # norm, coefficient
        gkey = self._bind(k, dev, params, grads)
        k.grad_sumsq(tree, ALL_BUCKETS, SLOT_GRAD, self._partials)
        k.norm_finish(self._partials, float(max_norm), out2)
        total_norm = out2[0]
        if error_if_nonfinite and not bool(torch.isfinite(total_norm)):
            raise RuntimeError(_NONFINITE)
        self._pending = (out2, gkey, grads)  # the tensors kept: their addresses stay theirs
        return total_norm

    def zero_grad(self, set_to_none: bool = True):
        """torch.optim.Optimizer.zero_grad; a clip coefficient still pending is dropped."""
        self._pending = None
        return super().zero_grad(set_to_none)

    @torch.no_grad()
    def step(self, closure=None):
        """One inner AdamW step (src/train.py:257), wrapped by torch.optim.Optimizer like every
        optimizer's step (profiler annotation, pre / post hooks)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        pending, self._pending = self._pending, None
        plan = self._fused_plan()
        if plan is None:
            if pending is not None:
                raise RuntimeError(
                    "InnerAdamW.step: a clip coefficient from clip_grad_norm_ is pending, but "
                    "this step cannot take the fused pass that applies it (see the class "
                    "docstring); the gradients are unscaled and nothing was stepped")
            # torch's own step body, unwrapped: this call already runs inside the hook wrapper
            inspect.unwrap(AdamW.step)(self)
            return loss
        k, dev, params, grads, scalars, states = plan
        coef = None
        if pending is not None:
            out2, gkey, _ = pending
            if gkey != tuple([gr.data_ptr() for gr in grads]):
                raise RuntimeError(
                    "InnerAdamW.step: the gradient tensors are not the ones clip_grad_norm_ "
                    "computed its pending coefficient from; nothing was stepped")
            coef = out2[1:]
        states = self._ensure_arenas(k, dev, params, states)
        self._bind(k, dev, params, grads)
        k.adamw_step(self._tree, ALL_BUCKETS, SLOT_INNER, SLOT_GRAD, self._m, self._v, scalars,
                     coef)
        torch._foreach_add_([s["step"] for s in states], 1)
        return loss
