"""Drop-in for the DiLoCo helpers of src/utils.py:203-226 and get_optimizer (src/utils.py:59-65).

Same names, arguments and host-visible results as the reference. Dispatch is on the inner
model's device, as the reference's `.to(param_outer.device)` / `.to(param_inner.device)`
copies are (src/utils.py:221,226): a GPU inner model runs the HIP path below; a CPU inner
model (the reference's --device cpu runs, tests/test_memorize.py:35-39) gets the reference's
per-tensor torch ops on the host. The GPU path has no CPU fallback: without libdiloco_hip.so
it raises. On the GPU:

  get_outer_model(inner)            deepcopy(inner).to("cpu")              src/utils.py:213-216
  compute_pseudo_gradient(in, out)  out.grad = out - in   (dl_delta_pack)   src/utils.py:218-221
  sync_inner_model(out, in)         in = out              (dl_scatter)      src/utils.py:223-226
  get_optimizer(model, cfg)         AdamW | SGD (outer: OuterSGD, HIP)      src/utils.py:59-65
  clip_grad_norm_(params, max_norm) torch's call at src/train.py:255 (dl_grad_sumsq ->
                                    dl_norm_finish -> dl_scale_by)

An AdamW outer optimizer (configs/optimizer/adamw.toml) is stock torch.optim.AdamW unless
DILOCO_OUTER_ADAMW=fused: then get_optimizer returns optim.OuterAdamW for an outer model, whose
step is one dl_delta_pack_adamw pass at one peer (36 B/param) and one dl_unpack_adamw pass per
bucket at N > 1; an outer model it is attached to takes the replicated exchange when none was
asked for. Asked for, the sharded exchange steps this rank's 1/n with dl_shard_adamw and the
rank-order one (DILOCO_DP_EXCHANGE=a2a) with dl_shard_reduce_adamw, exp_avg and exp_avg_sq
staying sharded until read. On the int8 wire (DILOCO_OUTER_WIRE=int8) every rank steps the whole
tree from the averaged slots, one dl_unpack_adamw_q8 pass per bucket. Anything its kernels do
not cover (amsgrad, tensor hyper-parameters, ...; see optim.OuterAdamW) runs torch's own step.

The inner optimizer (AdamW on a model that is not an outer model) is stock torch.optim.AdamW
unless DILOCO_INNER_ADAMW=fused: then get_optimizer returns optim.InnerAdamW, whose step is one
dl_adamw_step pass over the model's own tensors (28 B/param) after the clip above, or with the
clip folded in through InnerAdamW.clip_grad_norm_.

Placement of the outer model (`get_outer_model(..., placement=)`, default from the
DILOCO_OUTER_PLACEMENT environment variable, "host" if unset):

  "host"    the reference's placement: a CPU module whose parameters, gradients and momentum
            buffers hold exactly the reference's values whenever they are read. Write-back
            (`get_outer_model(..., write_back=)`, default from DILOCO_HOST_WRITEBACK):
              "lazy" (default)  the outer step runs on an HBM twin of the outer model
                        (mirror.LazyHostOuterMirror around a DeviceOuterMirror: the same
                        kernels and exchange as "device" below, no PCIe traffic per step);
                        the CPU tensors are views of pinned arenas refreshed from HBM when
                        something reads them (mirror.HostParameter / HostTensor), and host
                        writes are uploaded before the next call;
              "sync"    the host tensors are authoritative: every call ends with them
                        updated, one pinned DMA per arena (mirror.HostOuterMirror);
              "deferred"  as "sync", the step's write-back issued by sync_inner_model in one
                        batch of DMAs and not waited for (flush_outer_model / state_dict()
                        wait for it).
  "device"  SURVEY §8f row 2: the outer module lives on the inner model's GPU, its parameters,
            .grad and momentum buffers are views of packed HBM arenas
            (mirror.DeviceOuterMirror); host copies are made by torch on demand (`.cpu()`).

For "device" and "host"/"lazy": fused (`get_outer_model(..., fused=)`, DILOCO_OUTER_FUSED, on
if unset) runs the four calls as one HBM pass at one peer (dl_delta_pack_sgd) and as
pack -> exchange -> one SGD pass at N > 1, with .grad completing the deferred work when read
and sync_inner_model a verified no-op after the step; wire (DILOCO_OUTER_WIRE, "f32";
"bf16": BASELINE config #5's codec on the DP exchange; "int8": one scale per 4096-element
chunk, and with error_feedback (DILOCO_OUTER_Q8_EF, off if unset) both of its quantisers
carry what they round away into the next outer step: dl_delta_q8_ef, dl_q8_reduce_ef;
q8_error_feedback_state / load_q8_error_feedback_state; "fp4": the same exchange at 4 bits,
OCP MX block-scaled E2M1 in 2176-B slots, 0.531 B/param -- dl_delta_fp4, dl_fp4_reduce,
dl_unpack_sgd_fp4 / dl_unpack_adamw_fp4 -- with error_feedback from DILOCO_OUTER_FP4_EF, off if
unset, and the same two state helpers); exchange (DILOCO_OUTER_EXCHANGE;
"replicated", the host placement's default: all_reduce -> the SGD pass on every rank, so
.grad and the momentum are local on every rank as in the reference; "sharded", the device
placement's default: reduce_scatter -> SGD on this rank's 1/n -> all_gather of θ, SURVEY §8e;
"a2a": the sharded form with a rank-order sum, bit-exact at every n; DILOCO_DP_EXCHANGE=a2a
selects it too). Under the sharded forms a read of .grad or of the momentum buffers at N > 1
gathers them from the peers: a collective over the DP group that every rank must make; a read
its peers do not make raises RuntimeError after DILOCO_COLLECTIVE_READ_TIMEOUT seconds
(mirror.collective_read) instead of hanging.
"""
from __future__ import annotations

import copy
import os
from collections import OrderedDict

import torch
import torch.nn as nn
from torch.optim import SGD, AdamW, Optimizer

from .kernels import default_kernels
from .mirror import (DEFAULT_EXCHANGE, OUTER_EXCHANGES, OUTER_WIRES, SLOT_WIRES, WRITE_BACKS,
                     DeviceOuterMirror, HostOuterMirror, LazyHostOuterMirror, module_params)
from .optim import InnerAdamW, OuterAdamW, OuterSGD
from ._lib import ALL_BUCKETS
from .plan import DEFAULT_BUCKET_CAP_ELEMS, SLOT_GRAD

_ATTR = "_diloco_mirror"
_OUTER = "_diloco_outer"
_PLACEMENT = "_diloco_placement"
_WRITE_BACK = "_diloco_write_back"
_FUSED = "_diloco_fused"
_WIRE = "_diloco_wire"
_EXCHANGE = "_diloco_exchange"
_EXCHANGE_ASKED = "_diloco_exchange_asked"  # by argument or DILOCO_OUTER_EXCHANGE
_Q8_EF = "_diloco_q8_ef"  # int8 wire with error feedback (DILOCO_OUTER_Q8_EF)
_ADAMW = "_diloco_adamw"  # an optim.OuterAdamW is attached
OUTER_ADAMW = ("torch", "fused")
INNER_ADAMW = ("torch", "fused")  # DILOCO_INNER_ADAMW: the inner optimizer's step
_PENDING = "_diloco_pending_device"  # placement="device" built before the inner model moved
PLACEMENTS = ("host", "device")
_TRUE = ("1", "true", "on", "yes")
_FALSE = ("0", "false", "off", "no")


def env_flag(name: str, default: bool) -> bool:
    """A boolean knob from the environment: 1/0, true/false, on/off, yes/no (any case);
    anything else raises instead of silently meaning "on"."""
    v = os.environ.get(name)
    if v is None or v.strip() == "":
        return default
    v = v.strip().lower()
    if v in _TRUE:
        return True
    if v in _FALSE:
        return False
    raise ValueError(f"{name}={os.environ[name]!r}: one of {_TRUE + _FALSE}")


def device_path(t: torch.Tensor) -> bool:
    """True when tensors on t's device take the HIP path: device tensors always; host tensors
    only under a test backend that declares it computes on host tensors
    (tests/oracle_kernels.py: accepts_host_tensors, installed with set_default_kernels)."""
    return t.device.type != "cpu" or getattr(default_kernels(), "accepts_host_tensors", False)


def has_mirror(outer_model: nn.Module) -> bool:
    return getattr(outer_model, _ATTR, None) is not None


def _apply_adamw_mark(outer_model: nn.Module, m) -> None:
    """An outer model with an OuterAdamW attached and no exchange asked for takes the
    replicated exchange (the device placement's implicit sharded default does not apply):
    .grad, exp_avg and exp_avg_sq stay local on every rank, as torch's AdamW state is. The
    sharded and rank-order steps (their state reads are collectives) are for who asks."""
    dev = getattr(m, "dev", m)  # the lazy host mirror's HBM twin
    if hasattr(dev, "adamw_replicated"):
        dev.adamw_replicated = bool(getattr(outer_model, _ADAMW, False)
                                    and not getattr(outer_model, _EXCHANGE_ASKED, False))


def mark_adamw_outer(outer_model: nn.Module) -> None:
    """Called by optim.OuterAdamW at construction: the model's mirror (now or when it is
    created) sees the mark in all_reduce."""
    object.__setattr__(outer_model, _ADAMW, True)
    m = getattr(outer_model, _ATTR, None)
    if m is not None:
        _apply_adamw_mark(outer_model, m)


def outer_mirror(outer_model: nn.Module, device=None):
    """The device mirror of an outer model (created on first use): HostOuterMirror for the
    reference's host placement, DeviceOuterMirror for placement="device"."""
    m = getattr(outer_model, _ATTR, None)
    if m is None:
        k = default_kernels()
        # the int8 wire's error feedback is named only where it is on (off: the call as before)
        ef = {"error_feedback": True} if getattr(outer_model, _Q8_EF, False) else {}
        if getattr(outer_model, _PLACEMENT, "host") == "device":
            p = next(outer_model.parameters(), None)
            if p is None:
                raise ValueError("outer model has no parameters")
            keep = getattr(outer_model, _PENDING, False)
            dev = p.device
            if keep:  # the device is the inner model's, named now by the caller
                if device is None:
                    raise RuntimeError("the device outer model gets its device from the inner "
                                       "model's first compute_pseudo_gradient on the GPU")
                # its CPU parameters go straight into the HBM arena, tensor by tensor
                # (DeviceOuterMirror keep_params): no whole-model device copy first
                dev = torch.device(device)
                object.__setattr__(outer_model, _PENDING, False)
            cap = int(os.environ.get("DILOCO_OUTER_BUCKET_ELEMS", DEFAULT_BUCKET_CAP_ELEMS))
            m = DeviceOuterMirror(outer_model, dev, kernels=k, bucket_cap_elems=cap,
                                  fused=getattr(outer_model, _FUSED, False),
                                  wire=getattr(outer_model, _WIRE, "f32"),
                                  exchange=getattr(outer_model, _EXCHANGE,
                                                   DEFAULT_EXCHANGE["device"]),
                                  keep_params=keep, **ef)
            object.__setattr__(outer_model, _ATTR, m)
            _apply_adamw_mark(outer_model, m)
            return m
        if device is None:
            device = getattr(k, "default_device", None)
            if device is None:
                if not torch.cuda.is_available():
                    raise RuntimeError("the DiLoCo outer step runs on the GPU; no HIP device")
                device = torch.device("cuda", torch.cuda.current_device())
        wb = getattr(outer_model, _WRITE_BACK, "lazy")
        if wb == "lazy":
            cap = int(os.environ.get("DILOCO_OUTER_BUCKET_ELEMS", DEFAULT_BUCKET_CAP_ELEMS))
            m = LazyHostOuterMirror(outer_model, torch.device(device), kernels=k,
                                    bucket_cap_elems=cap,
                                    fused=getattr(outer_model, _FUSED, True),
                                    wire=getattr(outer_model, _WIRE, "f32"),
                                    exchange=getattr(outer_model, _EXCHANGE,
                                                     DEFAULT_EXCHANGE["host"]), **ef)
        else:
            m = HostOuterMirror(outer_model, torch.device(device), kernels=k, write_back=wb)
        object.__setattr__(outer_model, _ATTR, m)  # not a submodule / not in state_dict
        _apply_adamw_mark(outer_model, m)
    return m


def _inner_device(inner_model: nn.Module) -> torch.device:
    p = next(inner_model.parameters(), None)
    if p is None:
        raise ValueError("inner model has no parameters")
    return p.device


def get_outer_model(inner_model: nn.Module, placement: str = None,
                    write_back: str = None, fused: bool = None, wire: str = None,
                    exchange: str = None, error_feedback: bool = None) -> nn.Module:
    """Initializes the outer model from the inner model (src/utils.py:213-216).

    placement "host" (the reference's, default) or "device" (in HBM: on the inner model's GPU;
    built while the inner model is on the CPU, it stays there until the first
    compute_pseudo_gradient names the device); write_back "lazy" (default: the host outer
    model stepped on an HBM twin), "sync" or "deferred" for the host placement; fused
    (default on), wire ("f32" default, "bf16": BASELINE config #5's codec; "int8"; "fp4") and
    exchange ("replicated" for the host placement and "sharded" for placement="device" by
    default, or "a2a") for placement="device" and for the lazy host write-back (see the module
    docstring). error_feedback (int8 wire only; None reads DILOCO_OUTER_Q8_EF, default off):
    both quantisers of the int8 exchange carry what they round away into the next outer step
    (dl_delta_q8_ef, dl_q8_reduce_ef); q8_error_feedback_state / load_q8_error_feedback_state
    let a checkpoint carry the residuals. The fp4 wire takes error_feedback too (None reads
    DILOCO_OUTER_FP4_EF, default off): dl_delta_fp4 and dl_fp4_reduce with their residuals, the
    same arenas and the same two state helpers."""
    if placement is None:
        placement = os.environ.get("DILOCO_OUTER_PLACEMENT", "host")
    if placement not in PLACEMENTS:
        raise ValueError(f"placement {placement!r}: one of {PLACEMENTS}")
    if write_back is None:
        write_back = os.environ.get("DILOCO_HOST_WRITEBACK", "lazy")
    if write_back not in WRITE_BACKS:
        raise ValueError(f"write_back {write_back!r}: one of {WRITE_BACKS}")
    if fused is None:
        fused = env_flag("DILOCO_OUTER_FUSED", True)
    if wire is None:
        wire = os.environ.get("DILOCO_OUTER_WIRE", "f32")
    if wire not in OUTER_WIRES:
        raise ValueError(f"wire {wire!r}: one of {OUTER_WIRES}")
    if error_feedback is None:  # each variable is consulted for its own wire only
        error_feedback = ((wire == "int8" and env_flag("DILOCO_OUTER_Q8_EF", False))
                          or (wire == "fp4" and env_flag("DILOCO_OUTER_FP4_EF", False)))
    elif error_feedback and wire not in SLOT_WIRES:
        raise ValueError(f"error_feedback=True compensates the int8 / fp4 wire's quantiser; the "
                         f"wire is {wire!r}")
    if exchange is None:
        exchange = os.environ.get("DILOCO_OUTER_EXCHANGE") or None
    asked = exchange is not None
    if not asked:
        exchange = DEFAULT_EXCHANGE[placement]
    if exchange not in OUTER_EXCHANGES:
        raise ValueError(f"exchange {exchange!r}: one of {OUTER_EXCHANGES}")
    lazy = placement == "device" or write_back == "lazy"  # the outer step runs on an HBM copy
    if wire != "f32" and not lazy:
        raise ValueError("the bf16 outer wire needs placement='device' or write_back='lazy' "
                         "(write_back 'sync' / 'deferred' keep the host tensors authoritative)")
    outer_model = copy.deepcopy(inner_model)
    has_params = next(inner_model.parameters(), None) is not None
    if placement == "host":
        outer_model = outer_model.to("cpu")
    elif has_params:  # the inner model's GPU. The reference builds the outer model before it
        # moves the inner one to cuda:local_rank (src/train.py:382, :163, :368 with
        # src/utils.py:36-40) and never sets the current device: a CPU inner model leaves the
        # outer one on the CPU until the first compute_pseudo_gradient names the device
        # (outer_mirror; until then the four calls are the reference's host loops)
        dev = _inner_device(inner_model)
        if dev.type == "cpu" and device_path(next(inner_model.parameters())):
            # a test backend that computes on host tensors (tests/oracle_kernels.py)
            outer_model = outer_model.to(default_kernels().default_device)
        elif dev.type == "cpu":
            object.__setattr__(outer_model, _PENDING, True)
        else:
            outer_model = outer_model.to(dev)
    object.__setattr__(outer_model, _OUTER, True)  # get_optimizer: SGD here is the outer SGD
    object.__setattr__(outer_model, _PLACEMENT, placement)
    object.__setattr__(outer_model, _WRITE_BACK, write_back)
    object.__setattr__(outer_model, _FUSED, bool(fused) and lazy)
    object.__setattr__(outer_model, _WIRE, wire)
    object.__setattr__(outer_model, _Q8_EF, bool(error_feedback))
    object.__setattr__(outer_model, _EXCHANGE, exchange)
    object.__setattr__(outer_model, _EXCHANGE_ASKED, asked)
    if placement == "device" and has_params and not getattr(outer_model, _PENDING, False):
        # lay the parameters out in the packed HBM arena now (fused: as OuterParameters);
        # a model without parameters keeps none: the four calls are the reference's empty loops
        outer_mirror(outer_model)
    elif write_back == "lazy" and has_params and device_path(next(inner_model.parameters())):
        # the inner model is on its GPU already: the HBM twin now (the reference builds the
        # outer model before moving the inner one, src/train.py:382; then the first
        # compute_pseudo_gradient creates it)
        outer_mirror(outer_model, _inner_device(inner_model))
    elif write_back == "deferred":
        # a checkpoint of the outer model waits for the write-back in flight
        outer_model.register_state_dict_pre_hook(lambda mod, prefix, keep_vars:
                                                  flush_outer_model(mod))
    return outer_model


def _q8_ef_mirror(outer_model: nn.Module):
    m = getattr(outer_model, _ATTR, None)
    return getattr(m, "dev", m)  # the lazy host placement steps on its HBM twin's mirror


def q8_error_feedback_state(outer_model: nn.Module):
    """The int8 or fp4 wire's error-feedback residuals of this rank (both wires keep the same
    fp32 arenas, so one pair of helpers serves both), for a checkpoint:
    {"encode": the encoder's residual (packed layout), "reduce": [the residual of this rank's
    re-quantised slots, per bucket]} as clones. None when the feature is off or no exchange has
    run yet. The residuals are per rank (they are what this rank has not sent yet)."""
    m = _q8_ef_mirror(outer_model)
    if m is None or not getattr(m, "error_feedback", False):
        return None
    return m.q8_ef_state()


def load_q8_error_feedback_state(outer_model: nn.Module, state) -> None:
    """Copy a q8_error_feedback_state() back into an outer model built with the same tree,
    buckets and peer count (ValueError otherwise). None resets every residual to zero -- also
    the way out after a NaN/Inf pseudo-gradient left a non-finite residual."""
    m = _q8_ef_mirror(outer_model)
    if m is None or not getattr(m, "error_feedback", False):
        if state is None:
            return
        raise ValueError("this outer model has no int8 error feedback to load a state into "
                         "(the feature is off, or its device mirror is not built yet)")
    m.load_q8_ef_state(state)


def flush_outer_model(outer_model: nn.Module) -> None:
    """Make the host tensors of an outer model (parameters, .grad, momentum buffers) current:
    waits for a deferred write-back (a no-op for write_back="sync" and placement="device")."""
    m = getattr(outer_model, _ATTR, None)
    if m is not None:
        m.flush()


def _host_path(inner_model: nn.Module, outer_model: nn.Module) -> bool:
    """The reference's host semantics apply: a CPU inner model (or one without parameters,
    for which the reference's loops run zero times) and no device mirror."""
    p = next(inner_model.parameters(), None)
    return (p is None or not device_path(p)) and not has_mirror(outer_model)


def compute_pseudo_gradient(inner_model: nn.Module, outer_model: nn.Module) -> None:
    """outer.grad = outer - inner for every parameter (src/utils.py:218-221)."""
    m = getattr(outer_model, _ATTR, None)
    if m is not None:  # every call after the first: straight to the mirror
        m.pseudo_gradient(module_params(inner_model))
        return
    if _host_path(inner_model, outer_model):
        with torch.no_grad():
            for po, pi in zip(outer_model.parameters(), inner_model.parameters()):
                po.grad = torch.sub(po.data, pi.data.to(po.device))  # a fresh tensor
        return
    dev = _inner_device(inner_model)
    m = outer_mirror(outer_model, dev if dev.type != "cpu" else None)
    m.pseudo_gradient(module_params(inner_model))


def sync_inner_model(outer_model: nn.Module, inner_model: nn.Module) -> None:
    """inner = outer for every parameter (src/utils.py:223-226)."""
    m = getattr(outer_model, _ATTR, None)
    if m is not None:
        m.copy_to_inner(module_params(inner_model))
        return
    if _host_path(inner_model, outer_model):
        with torch.no_grad():
            for po, pi in zip(outer_model.parameters(), inner_model.parameters()):
                pi.data.copy_(po.data.to(pi.device))
        return
    dev = _inner_device(inner_model)
    m = outer_mirror(outer_model, dev if dev.type != "cpu" else None)
    m.copy_to_inner(module_params(inner_model))


# clip_grad_norm_'s trees: one per (backend, device, gradient sizes) seen; a training run has one
# or two (a model, a pipeline stage). Bounded: the least recently used tree is closed.
CLIP_CACHE_SIZE = 4
_clip_cache: "OrderedDict[tuple, tuple]" = OrderedDict()


def _clip_tree(k, device: torch.device, numels: tuple):
    """(PackedTree over the gradients' sizes, its per-chunk partial sums), cached."""
    key = (k.name, device, numels)
    hit = _clip_cache.get(key)
    if hit is not None:
        _clip_cache.move_to_end(key)
        return hit
    tree = k.tree(numels, device)
    partials = torch.zeros(max(1, tree.n_chunks), dtype=torch.float64, device=device)
    _clip_cache[key] = (tree, partials)
    while len(_clip_cache) > CLIP_CACHE_SIZE:
        _, (old, _) = _clip_cache.popitem(last=False)
        old.close()
    return tree, partials


def clip_grad_norm_(parameters, max_norm: float, norm_type: float = 2.0,
                    error_if_nonfinite: bool = False, foreach=None) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_ (src/train.py:255): same arguments, same return.

    The 2-norm of fp32, contiguous gradients on one GPU runs as three HIP launches on the
    current stream: dl_grad_sumsq (one read of every gradient, fp64 sums in a fixed order) ->
    dl_norm_finish (norm and torch's fp32 clip coefficient, on the device) -> dl_scale_by
    (g *= coef; touches no memory when nothing is clipped). No host synchronisation unless
    error_if_nonfinite asks for the norm's value. Differences from torch: the norm is the
    correctly rounded fp32 of an fp64 sum (within 2^-23 of torch's, relative), and it stays
    finite where torch's fp32 accumulation overflows (|g| >~ 1.8e19). Anything else -- CPU
    gradients, another norm_type, other dtypes, several devices -- is torch's own call."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    else:
        parameters = list(parameters)
    grads = [p.grad for p in parameters if p.grad is not None]
    if not (grads and float(norm_type) == 2.0 and device_path(grads[0]) and all(
            g.dtype == torch.float32 and g.is_contiguous() and g.device == grads[0].device
            and g.layout == torch.strided for g in grads)):
        return torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type,
                                              error_if_nonfinite, foreach)
    k = default_kernels()
    device = grads[0].device
    with torch.no_grad():
        tree, partials = _clip_tree(k, device, tuple(g.numel() for g in grads))
        out2 = torch.empty(2, dtype=torch.float32, device=device)  # norm, coefficient
        k.bind(tree, SLOT_GRAD, grads, device)  # .grad is reallocated every step
        k.grad_sumsq(tree, ALL_BUCKETS, SLOT_GRAD, partials)
        k.norm_finish(partials, float(max_norm), out2)
        total_norm = out2[0]
        if error_if_nonfinite and not bool(torch.isfinite(total_norm)):
            raise RuntimeError(
                f"The total norm of order {float(norm_type)} for gradients from "
                "`parameters` is non-finite, so it cannot be clipped. To disable "
                "this error and scale the gradients by the non-finite norm anyway, "
                "set `error_if_nonfinite=False`")
        k.scale_by(tree, ALL_BUCKETS, SLOT_GRAD, out2[1:])
    return total_norm


def get_optimizer(model: nn.Module, optimizer_config) -> Optimizer:
    """src/utils.py:59-65. SGD on the outer model (from get_outer_model) -> OuterSGD; AdamW on
    it under DILOCO_OUTER_ADAMW=fused -> OuterAdamW (unset or "torch": stock AdamW). AdamW on
    any other model (the inner optimizer, src/train.py:418) under DILOCO_INNER_ADAMW=fused ->
    InnerAdamW (unset or "torch": stock AdamW)."""
    if optimizer_config.type == "AdamW":
        knob = (os.environ.get("DILOCO_OUTER_ADAMW") or "torch").strip().lower()
        if knob not in OUTER_ADAMW:
            raise ValueError(f"DILOCO_OUTER_ADAMW={knob!r}: one of {OUTER_ADAMW}")
        inner_knob = (os.environ.get("DILOCO_INNER_ADAMW") or "torch").strip().lower()
        if inner_knob not in INNER_ADAMW:
            raise ValueError(f"DILOCO_INNER_ADAMW={inner_knob!r}: one of {INNER_ADAMW}")
        if knob == "fused" and getattr(model, _OUTER, False):
            return OuterAdamW(model, lr=optimizer_config.lr,
                              weight_decay=optimizer_config.weight_decay,
                              betas=optimizer_config.betas)
        if inner_knob == "fused" and not getattr(model, _OUTER, False):
            return InnerAdamW(model.parameters(), lr=optimizer_config.lr,
                              weight_decay=optimizer_config.weight_decay,
                              betas=optimizer_config.betas)
        return AdamW(model.parameters(), lr=optimizer_config.lr,
                     weight_decay=optimizer_config.weight_decay, betas=optimizer_config.betas)
    elif optimizer_config.type == "SGD":
        if getattr(model, _OUTER, False):
            return OuterSGD(model, lr=optimizer_config.lr, momentum=optimizer_config.momentum,
                            nesterov=optimizer_config.nesterov)
        return SGD(model.parameters(), lr=optimizer_config.lr, momentum=optimizer_config.momentum,
                   nesterov=optimizer_config.nesterov)
    else:
        raise ValueError(f"Invalid optimizer type: {optimizer_config.type}")
