"""The kernel backend of the outer-step engines: libdiloco_hip.so through its C-ABI.

Every engine (OuterSync, GradSync, HostOuterMirror) calls these methods and nothing else for
compute, so the orchestration above them (bucketing, pipelining, /n, optimizer state) is one
code path. `HipKernels` is the only backend the package ships; it launches on the current
HIP stream of the tensors' device and raises if the library or the GPU is missing.
"""
from __future__ import annotations

import ctypes

from typing import Optional, Sequence

import torch

from . import _lib
from .plan import DEFAULT_BUCKET_CAP_ELEMS, PackedTree

_DT = {torch.float32: _lib.DL_F32, torch.bfloat16: _lib.DL_BF16}


Q8_SLOT = _lib.Q8_SLOT_BYTES
FP4_SLOT = _lib.FP4_SLOT_BYTES


def wire_code(dtype: torch.dtype) -> int:
    try:
        return _DT[dtype]
    except KeyError:
        raise TypeError(f"unsupported packed dtype {dtype} (float32 or bfloat16)") from None


def adamw_scalars(lr: float, beta1: float, beta2: float, weight_decay: float, eps: float,
                  step: float) -> tuple:
    """The seven per-step scalars of the dl_*_adamw entry points (decay, w1, beta2,
    w2, neg_step_size, bc2_sqrt, eps) in Python doubles, each expression written as torch's
    _single_tensor_adamw writes it; `step` is the count after this step. The C-ABI call narrows
    each to fp32 once, as torch does when the Python scalar meets the fp32 tensor."""
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    step_size = lr / bias_correction1
    return (1 - lr * weight_decay, 1 - beta1, beta2, 1 - beta2, -step_size,
            bias_correction2 ** 0.5, eps)


def _s(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


class HipKernels:
    """Segment-walker kernels of libdiloco_hip.so (DESIGN.md "Kernels")."""

    name = "hip"

    def check_device(self, device: torch.device) -> None:
        if device.type != "cuda":
            raise ValueError(f"the HIP outer-step kernels need device tensors, got {device}")
        _lib.load()

    def tree(self, numels: Sequence[int], device: torch.device,
             cap_elems: int = DEFAULT_BUCKET_CAP_ELEMS,
             bucket_align: int = _lib.ALIGN_ELEMS) -> PackedTree:
        self.check_device(device)
        with torch.cuda.device(device):
            return PackedTree(numels, cap_elems, bucket_align)

    def bind(self, tree: PackedTree, slot: int, tensors: Sequence[torch.Tensor], device,
             key=None) -> None:
        """key: tuple of the tensors' addresses, if the caller computed it (skips a pass)."""
        if key is not None and tree._bound[slot] == key:
            return
        tree.bind(slot, tensors, torch.cuda.current_stream(device).cuda_stream, key)

    def delta_pack(self, tree, bucket, inner_slot, theta, wire) -> None:
        _lib.call("dl_delta_pack", tree.handle, bucket, inner_slot, theta.data_ptr(),
                  wire.data_ptr(), wire_code(wire.dtype), _s(theta))

    def unpack_sgd(self, tree, bucket, wire, divisor, theta, mom, lr, momentum, nesterov,
                   first, inner_slot) -> None:
        _lib.call("dl_unpack_sgd", tree.handle, bucket, wire.data_ptr(), wire_code(wire.dtype),
                  int(divisor), theta.data_ptr(), _ptr(mom), float(lr), float(momentum),
                  int(nesterov), int(first), int(inner_slot), _s(theta))

    def unpack_sgd_merge(self, tree, bucket, wire, divisor, theta, mom, lr, momentum, nesterov,
                         first, inner_slot, alpha) -> None:
        """unpack_sgd whose inner write merges: inner <- fma(alpha, inner - θ, θ), one pass
        (0 <= alpha < 1; alpha 0 is unpack_sgd; inner_slot must be bound)."""
        _lib.call("dl_unpack_sgd_merge", tree.handle, bucket, wire.data_ptr(),
                  wire_code(wire.dtype), int(divisor), theta.data_ptr(), _ptr(mom), float(lr),
                  float(momentum), int(nesterov), int(first), int(inner_slot), float(alpha),
                  _s(theta))

    def delta_sgd(self, tree, bucket, inner_slot, theta, mom, lr, momentum, nesterov,
                  first) -> None:
        _lib.call("dl_delta_sgd", tree.handle, bucket, inner_slot, theta.data_ptr(), _ptr(mom),
                  float(lr), float(momentum), int(nesterov), int(first), _s(theta))

    def delta_pack_sgd(self, tree, bucket, inner_slot, theta, wire, mom, lr, momentum, nesterov,
                       first) -> None:
        """One peer, one pass: delta + SGD + copy-back, the pseudo-gradient kept in `wire`."""
        _lib.call("dl_delta_pack_sgd", tree.handle, bucket, inner_slot, theta.data_ptr(),
                  wire.data_ptr(), wire_code(wire.dtype), _ptr(mom), float(lr), float(momentum),
                  int(nesterov), int(first), _s(theta))

    def delta_pack_sgd_defer(self, tree, bucket, inner_slot, theta, wire, mom, lr, momentum,
                             nesterov, first) -> None:
        """delta_pack_sgd (fp32 wire) without the stores of θ and the momentum: the step stays
        pending in (theta, mom, wire) until unpack_sgd(divisor 1, inner_slot -1) with the same
        hyper-parameters, or delta_pack_sgd_resume, completes it."""
        _lib.call("dl_delta_pack_sgd_defer", tree.handle, bucket, inner_slot, theta.data_ptr(),
                  wire.data_ptr(), _ptr(mom), float(lr), float(momentum), int(nesterov),
                  int(first), _s(theta))

    def delta_pack_sgd_resume(self, tree, bucket, inner_slot, theta, wire, mom, pending, lr,
                              momentum, nesterov, first) -> None:
        """The step after a pending one (pending: its lr, momentum, nesterov, first): that
        step redone in registers, then delta_pack_sgd; theta, mom, wire and inner stored."""
        p_lr, p_momentum, p_nesterov, p_first = pending
        _lib.call("dl_delta_pack_sgd_resume", tree.handle, bucket, inner_slot, theta.data_ptr(),
                  wire.data_ptr(), _ptr(mom), float(p_lr), float(p_momentum), int(p_nesterov),
                  int(p_first), float(lr), float(momentum), int(nesterov), int(first), _s(theta))

    def unpack_adamw(self, tree, bucket, wire, divisor, theta, exp_avg, exp_avg_sq, scalars,
                     inner_slot) -> None:
        """N > 1: the summed wire / divisor, then one AdamW step on θ, exp_avg, exp_avg_sq
        (and the inner params); scalars from adamw_scalars."""
        _lib.call("dl_unpack_adamw", tree.handle, bucket, wire.data_ptr(), wire_code(wire.dtype),
                  int(divisor), theta.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                  *scalars, int(inner_slot), _s(theta))

    def unpack_adamw_merge(self, tree, bucket, wire, divisor, theta, exp_avg, exp_avg_sq, scalars,
                           inner_slot, alpha) -> None:
        """unpack_adamw with unpack_sgd_merge's inner write."""
        _lib.call("dl_unpack_adamw_merge", tree.handle, bucket, wire.data_ptr(),
                  wire_code(wire.dtype), int(divisor), theta.data_ptr(), exp_avg.data_ptr(),
                  exp_avg_sq.data_ptr(), *scalars, int(inner_slot), float(alpha), _s(theta))

    def delta_pack_adamw(self, tree, bucket, inner_slot, theta, wire, exp_avg, exp_avg_sq,
                         scalars) -> None:
        """One peer, one pass: delta + AdamW + copy-back, the pseudo-gradient kept in `wire`."""
        _lib.call("dl_delta_pack_adamw", tree.handle, bucket, inner_slot, theta.data_ptr(),
                  wire.data_ptr(), wire_code(wire.dtype), exp_avg.data_ptr(),
                  exp_avg_sq.data_ptr(), *scalars, _s(theta))

    def adamw_step(self, tree, bucket, param_slot, grad_slot, exp_avg, exp_avg_sq, scalars,
                   coef=None) -> None:
        """The inner AdamW step, one pass on the current stream: θ in place in the bound
        param_slot, g read from the bound grad_slot (times coef[0], a device scalar, when
        given: the gradients stay unscaled), exp_avg / exp_avg_sq packed arenas in the tree's
        layout; scalars from adamw_scalars."""
        _lib.call("dl_adamw_step", tree.handle, bucket, int(param_slot), int(grad_slot),
                  exp_avg.data_ptr(), exp_avg_sq.data_ptr(), _ptr(coef), *scalars, _s(exp_avg))

    def pack_sgd_tiled(self, tree, bucket, inner_slot, theta, wire, mom, lr, momentum,
                       nesterov, first, tile_chunks) -> None:
        """One peer: delta_pack then unpack_sgd (divisor 1) tile by tile (Infinity-Cache
        blocking); the same results as the two whole-range launches."""
        _lib.call("dl_pack_sgd_tiled", tree.handle, bucket, inner_slot, theta.data_ptr(),
                  wire.data_ptr(), wire_code(wire.dtype), _ptr(mom), float(lr), float(momentum),
                  int(nesterov), int(first), int(tile_chunks), _s(theta))

    def shard_sgd(self, wire, divisor, theta, mom, lr, momentum, nesterov, first) -> None:
        """Flat 1/n shard after a reduce-scatter (wire, theta, mom: equal-length views)."""
        _lib.call("dl_shard_sgd", wire.data_ptr(), wire_code(wire.dtype), int(divisor),
                  theta.data_ptr(), _ptr(mom), theta.numel(), float(lr), float(momentum),
                  int(nesterov), int(first), _s(theta))

    def shard_reduce_sgd(self, slices, n_slices, theta, mom, lr, momentum, nesterov,
                         first) -> None:
        """Flat 1/n shard after an all_to_all: slices = n_slices equal slices (wire dtype) of
        theta's length; Σ in rank order, /n, SGD on theta / mom (equal-length views)."""
        _lib.call("dl_shard_reduce_sgd", slices.data_ptr(), wire_code(slices.dtype),
                  int(n_slices), theta.numel(), theta.data_ptr(), _ptr(mom), float(lr),
                  float(momentum), int(nesterov), int(first), _s(theta))

    def shard_reduce_avg(self, slices, n_slices, out) -> None:
        """out = Σ of the n_slices equal slices in rank order / n (fp32 out, out's length)."""
        _lib.call("dl_shard_reduce_avg", slices.data_ptr(), wire_code(slices.dtype),
                  int(n_slices), out.numel(), out.data_ptr(), _s(out))

    def shard_adamw(self, wire, divisor, theta, exp_avg, exp_avg_sq, scalars) -> None:
        """Flat 1/n shard after a reduce-scatter: wire / divisor, then one AdamW step on theta,
        exp_avg, exp_avg_sq (equal-length views); scalars from adamw_scalars."""
        _lib.call("dl_shard_adamw", wire.data_ptr(), wire_code(wire.dtype), int(divisor),
                  theta.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), theta.numel(),
                  *scalars, _s(theta))

    def shard_reduce_adamw(self, slices, n_slices, theta, exp_avg, exp_avg_sq, scalars,
                           avg_out=None) -> None:
        """Flat 1/n shard after an all_to_all: slices = n_slices equal slices (wire dtype) of
        theta's length; Σ in rank order, /n (kept in avg_out, fp32, if given), then one AdamW
        step on theta, exp_avg, exp_avg_sq (equal-length views)."""
        _lib.call("dl_shard_reduce_adamw", slices.data_ptr(), wire_code(slices.dtype),
                  int(n_slices), theta.numel(), theta.data_ptr(), exp_avg.data_ptr(),
                  exp_avg_sq.data_ptr(), _ptr(avg_out), *scalars, _s(theta))

    def xgmi_reduce_sgd(self, wires, thetas, n, rank, lo, length, mom, lr, momentum, nesterov,
                        first, device=None) -> None:
        """Direct exchange on this rank's shard (wires / thetas: uint64 arrays of the n peers'
        device addresses, IPC-mapped)."""
        p64 = ctypes.POINTER(ctypes.c_uint64)
        _lib.call("dl_xgmi_reduce_sgd", wires.ctypes.data_as(p64), thetas.ctypes.data_as(p64),
                  int(n), int(rank), int(lo), int(length), _ptr(mom), float(lr),
                  float(momentum), int(nesterov), int(first),
                  torch.cuda.current_stream(device).cuda_stream)

    def xgmi_delta_sgd(self, inners, thetas, n, rank, lo, length, mom, lr, momentum, nesterov,
                       first, device=None) -> None:
        """Direct exchange from the peers' packed inner arenas (no wire): g formed in-kernel."""
        p64 = ctypes.POINTER(ctypes.c_uint64)
        _lib.call("dl_xgmi_delta_sgd", inners.ctypes.data_as(p64), thetas.ctypes.data_as(p64),
                  int(n), int(rank), int(lo), int(length), _ptr(mom), float(lr),
                  float(momentum), int(nesterov), int(first),
                  torch.cuda.current_stream(device).cuda_stream)

    def sys_fence(self, device=None) -> None:
        """L2 write-back + invalidate on every XCD (cross-GPU ordering of IPC-shared buffers)."""
        _lib.call("dl_sys_fence", torch.cuda.current_stream(device).cuda_stream)

    # int8 wire codec (DL_Q8_SLOT_BYTES slots, one per chunk)
    def delta_q8(self, tree, bucket, inner_slot, theta, slots) -> None:
        _lib.call("dl_delta_q8", tree.handle, bucket, inner_slot, theta.data_ptr(),
                  slots.data_ptr(), _s(theta))

    def q8_reduce(self, recv, n_peers, n_slots, divisor, out) -> None:
        _lib.call("dl_q8_reduce", recv.data_ptr(), int(n_peers), int(n_slots), int(divisor),
                  out.data_ptr(), _s(out))

    def delta_q8_ef(self, tree, bucket, inner_slot, theta, residual, slots) -> None:
        """delta_q8 with error feedback: x = (θ - inner) + residual is quantised and
        residual <- x - q·s in place (fp32, the tree's packed layout)."""
        _lib.call("dl_delta_q8_ef", tree.handle, bucket, inner_slot, theta.data_ptr(),
                  residual.data_ptr(), slots.data_ptr(), _s(theta))

    def q8_reduce_ef(self, recv, n_peers, n_slots, divisor, residual, out) -> None:
        """q8_reduce with the shard owner's residual (n_slots * CHUNK_ELEMS floats) added to the
        average before it is re-quantised, and rewritten in place."""
        _lib.call("dl_q8_reduce_ef", recv.data_ptr(), int(n_peers), int(n_slots), int(divisor),
                  residual.data_ptr(), out.data_ptr(), _s(out))

    def unpack_sgd_q8(self, tree, bucket, slots, theta, mom, lr, momentum, nesterov, first,
                      inner_slot) -> None:
        _lib.call("dl_unpack_sgd_q8", tree.handle, bucket, slots.data_ptr(), theta.data_ptr(),
                  _ptr(mom), float(lr), float(momentum), int(nesterov), int(first),
                  int(inner_slot), _s(theta))

    def unpack_adamw_q8(self, tree, bucket, slots, theta, exp_avg, exp_avg_sq, scalars,
                        inner_slot) -> None:
        """The averaged int8 slots of a bucket: g = q·s, then one AdamW step on θ, exp_avg,
        exp_avg_sq (and the inner params), as unpack_adamw on the decoded values; scalars from
        adamw_scalars."""
        _lib.call("dl_unpack_adamw_q8", tree.handle, bucket, slots.data_ptr(), theta.data_ptr(),
                  exp_avg.data_ptr(), exp_avg_sq.data_ptr(), *scalars, int(inner_slot),
                  _s(theta))

    # fp4 (MXFP4) wire codec (DL_FP4_SLOT_BYTES slots, one per chunk; dl_fp4.hip). residual
    # None: no error feedback
    def delta_fp4(self, tree, bucket, inner_slot, theta, residual, slots) -> None:
        """slots <- enc(x), x = θ - inner (+ residual); residual <- x - deq(slots) in place."""
        _lib.call("dl_delta_fp4", tree.handle, bucket, inner_slot, theta.data_ptr(),
                  _ptr(residual), slots.data_ptr(), _s(theta))

    def fp4_reduce(self, recv, n_peers, n_slots, divisor, residual, out) -> None:
        """out <- enc((Σ_r deq(recv[r])) / divisor (+ residual)), r in rank order; residual (the
        owner's n_slots * CHUNK_ELEMS floats) rewritten in place."""
        _lib.call("dl_fp4_reduce", recv.data_ptr(), int(n_peers), int(n_slots), int(divisor),
                  _ptr(residual), out.data_ptr(), _s(out))

    def unpack_sgd_fp4(self, tree, bucket, slots, theta, mom, lr, momentum, nesterov, first,
                       inner_slot) -> None:
        _lib.call("dl_unpack_sgd_fp4", tree.handle, bucket, slots.data_ptr(), theta.data_ptr(),
                  _ptr(mom), float(lr), float(momentum), int(nesterov), int(first),
                  int(inner_slot), _s(theta))

    def unpack_adamw_fp4(self, tree, bucket, slots, theta, exp_avg, exp_avg_sq, scalars,
                         inner_slot) -> None:
        _lib.call("dl_unpack_adamw_fp4", tree.handle, bucket, slots.data_ptr(), theta.data_ptr(),
                  exp_avg.data_ptr(), exp_avg_sq.data_ptr(), *scalars, int(inner_slot),
                  _s(theta))

    # the gradient side of the int8 exchange (dl_q8_grad.hip)
    def gather_q8(self, tree, bucket, src_slot, slots) -> None:
        """slots <- quantise(the gradients bound to src_slot), one slot per chunk."""
        _lib.call("dl_gather_q8", tree.handle, bucket, int(src_slot), slots.data_ptr(), _s(slots))

    def gather_q8_ef(self, tree, bucket, src_slot, residual, slots) -> None:
        """gather_q8 with error feedback: x = g + residual is quantised and
        residual <- x - q·s in place (fp32, the tree's packed layout)."""
        _lib.call("dl_gather_q8_ef", tree.handle, bucket, int(src_slot), residual.data_ptr(),
                  slots.data_ptr(), _s(slots))

    def unpack_avg_q8(self, tree, bucket, slots, dst_slot, partials=None) -> None:
        """dst_slot <- q·s of the averaged slots; with partials also the per-chunk Σ of the
        stored values² (grad_sumsq's, for norm_finish)."""
        _lib.call("dl_unpack_avg_q8", tree.handle, bucket, slots.data_ptr(), int(dst_slot),
                  _ptr(partials), _s(slots))

    # the gradient side of the fp4 exchange (dl_fp4_grad.hip). residual None: no error feedback
    def gather_fp4(self, tree, bucket, src_slot, residual, slots) -> None:
        """slots <- enc(x), x = the gradients bound to src_slot (+ residual);
        residual <- x - deq(slots) in place (fp32, the tree's packed layout)."""
        _lib.call("dl_gather_fp4", tree.handle, bucket, int(src_slot), _ptr(residual),
                  slots.data_ptr(), _s(slots))

    def unpack_avg_fp4(self, tree, bucket, slots, dst_slot, partials=None) -> None:
        """dst_slot <- deq of the averaged slots; with partials also the per-chunk Σ of the
        stored values² (grad_sumsq's, for norm_finish)."""
        _lib.call("dl_unpack_avg_fp4", tree.handle, bucket, slots.data_ptr(), int(dst_slot),
                  _ptr(partials), _s(slots))

    def unpack_avg(self, tree, bucket, wire, divisor, dst_slot, dst_packed=None) -> None:
        _lib.call("dl_unpack_avg", tree.handle, bucket, wire.data_ptr(), wire_code(wire.dtype),
                  int(divisor), int(dst_slot), _ptr(dst_packed), _s(wire))

    # gradient-norm clipping (dl_norm.hip): partials = tree.n_chunks doubles, out2 = 2 floats
    def grad_sumsq(self, tree, bucket, src_slot, partials) -> None:
        """partials[c] = Σ g² over each chunk c of the bucket, in fp64."""
        _lib.call("dl_grad_sumsq", tree.handle, bucket, int(src_slot), partials.data_ptr(),
                  _s(partials))

    def unpack_avg_sumsq(self, tree, bucket, wire, divisor, dst_slot, partials,
                         dst_packed=None) -> None:
        """unpack_avg that also leaves partials[c] of the values it stores."""
        _lib.call("dl_unpack_avg_sumsq", tree.handle, bucket, wire.data_ptr(),
                  wire_code(wire.dtype), int(divisor), int(dst_slot), _ptr(dst_packed),
                  partials.data_ptr(), _s(wire))

    def norm_finish(self, partials, max_norm, out2) -> None:
        """out2[0] = the 2-norm from the partial sums, out2[1] = torch's clip coefficient."""
        _lib.call("dl_norm_finish", partials.data_ptr(), partials.numel(), float(max_norm),
                  out2.data_ptr(), _s(out2))

    def scale_by(self, tree, bucket, slot, coef) -> None:
        """slot *= coef[0] (a device scalar) in place; no memory touched when it is 1."""
        _lib.call("dl_scale_by", tree.handle, bucket, int(slot), coef.data_ptr(), _s(coef))

    def gather(self, tree, bucket, src_slot, packed) -> None:
        _lib.call("dl_gather", tree.handle, bucket, src_slot, packed.data_ptr(),
                  wire_code(packed.dtype), _s(packed))

    def scatter(self, tree, bucket, packed, dst_slot) -> None:
        _lib.call("dl_scatter", tree.handle, bucket, packed.data_ptr(), dst_slot, _s(packed))


_DEFAULT = None


def default_kernels():
    """The backend the engines use: HipKernels unless a test installed its own checker
    backend with set_default_kernels (tests/oracle_kernels.py; never done by the package)."""
    global _DEFAULT
    if _DEFAULT is None:
        _DEFAULT = HipKernels()
    return _DEFAULT


def set_default_kernels(k) -> None:
    """Test hook: route the engines through `k` (None restores HipKernels)."""
    global _DEFAULT
    _DEFAULT = k
