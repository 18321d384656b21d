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
"""
from __future__ import annotations

import inspect
from operator import is_, methodcaller

import torch
from torch.optim import SGD, AdamW

from .kernels import adamw_scalars
from .mirror import HostOuterMirror

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
    followed by the all_gather of θ. It IS a torch.optim.AdamW (param_groups, hooks, LR
    schedulers and state_dict work unchanged; state[p]["step"] is torch's fp32 scalar tensor,
    exp_avg and exp_avg_sq are views of the mirror's packed arenas), selected by get_optimizer
    under DILOCO_OUTER_ADAMW=fused. After a sharded or rank-order step each rank holds its own
    1/n of exp_avg and exp_avg_sq; reading either, or state_dict(), gathers the rest first -- a
    collective over the DP group, like reading the momentum of a sharded OuterSGD.

    The fused pass is one element of torch's _single_tensor_adamw (include/diloco_hip.h).
    Whenever that contract or the mirror does not cover the step -- amsgrad, maximize,
    capturable, differentiable, beta1 <= 0.5, tensor hyper-parameters, more than one group,
    parameters whose step counts differ, the int8 exchange, write_back "sync" or
    "deferred", no mirror at all (a CPU-only run) -- step() runs torch's own step body, exactly
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
