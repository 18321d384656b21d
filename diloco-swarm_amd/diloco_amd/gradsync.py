"""DP average of device gradients: the reference's per-tensor loop in one bucketed pass.

`TrainingComm.sync_gradients(model)` (src/comm.py:117-123) on a model whose gradients live on
the GPU -- plain DP / SWARM without an outer optimizer, called every sync step at
src/train.py:249-251:

    for p in model.parameters():
        all_reduce(p.grad, SUM); p.grad /= num_peers

becomes, per bucket: dl_gather (grads -> packed wire) -> RCCL all_reduce(SUM) ->
dl_unpack_avg (wire / n -> grads), pipelined across buckets (outer.pipelined_buckets).

exchange="a2a" (as OuterSync's): per bucket dl_gather -> RCCL all_to_all of the wire slices ->
dl_shard_reduce_avg (Σ in rank order in fp32, / n, into this peer's shard) -> RCCL all_gather
of the averaged shards -> dl_unpack_avg (a copy): the same bus bytes as the all-reduce, an
average that does not depend on RCCL's algorithm and is bit-exact against oracle/or_sum_avg at
every n.

wire_dtype=torch.int8: the int8 wire of the outer step (dl_q8.hip; one DL_Q8_SLOT_BYTES slot
per chunk, bucket b's slots padded with zero slots to a multiple of the peer count; plan.
q8_slot_plan) on the exchange that runs every step -- per bucket dl_gather_q8 -> RCCL all_to_all
of the slots -> dl_q8_reduce (Σ of the peers' dequantised slots in rank order, / n, re-quantised)
-> RCCL all_gather -> dl_unpack_avg_q8 (q·s into .grad): 2(n-1)/n · 1.016 bus bytes per
parameter against 8(n-1)/n, every peer left with byte-identical gradients. error_feedback=True:
dl_gather_q8_ef and dl_q8_reduce_ef in their places -- what each quantiser rounds away is added
to the next step's value (q_residual, 4 B/param; q_residual_red, 4/n B/param; both stay on
this peer; q8_ef_state / load_q8_ef_state). One replica: encode, the plain in-place re-quantise,
decode -- only the encoder's residual. A NaN/Inf gradient leaves a non-finite residual (IEEE
rules, as in the outer codec) until load_q8_ef_state(None) resets it. The residuals belong to
this GradSync: one rebuilt for other parameters starts from zero.

wire_dtype="fp4" (the string: no torch dtype names the format on every build): the same slot
exchange with the outer step's 4-bit codec (dl_fp4.hip; one DL_FP4_SLOT_BYTES slot per chunk, the
same slot plan) -- per bucket dl_gather_fp4 -> all_to_all -> dl_fp4_reduce (divisor n) ->
all_gather -> dl_unpack_avg_fp4: 2(n-1)/n · 0.531 bus bytes per parameter. error_feedback=True
hands the same two residual arenas to dl_gather_fp4 and dl_fp4_reduce (q8_ef_state /
load_q8_ef_state serve both slot wires). One replica: encode, dl_fp4_reduce of the region onto
itself (the identity: deq(enc(deq(s))) == deq(s)), decode. The two slot wires differ in their
slot size and their three calls only (SLOT_WIRES).

sync(max_norm): the clip_grad_norm_ that follows the sync in the training loop
(src/train.py:255), fused into it. Every dl_unpack_avg becomes dl_unpack_avg_sumsq, which holds
each averaged gradient in registers on its way to .grad and leaves the chunk's Σ g²; after the
last bucket dl_norm_finish and one dl_scale_by run on the same stream (int8 wire:
dl_unpack_avg_q8, fp4 wire: dl_unpack_avg_fp4 leave the same partial sums). Equal, bit for bit, to
sync() followed by utils.clip_grad_norm_, without that call's read of every gradient.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
import torch.distributed as dist

from .kernels import FP4_SLOT, Q8_SLOT, default_kernels
from . import _lib
from .outer import _Done, pipelined_buckets
from .plan import DEFAULT_BUCKET_CAP_ELEMS, SLOT_GRAD, q8_slot_plan


# The slot wires: wire_dtype -> slot bytes. Each has a three-call codec (encode, reduce, decode;
# GradSync._codec), as the mirror's SLOT_WIRES; everything between the calls is shared.
SLOT_WIRES = {torch.int8: Q8_SLOT, "fp4": FP4_SLOT}


class GradSync:
    def __init__(self, params: Sequence[torch.Tensor], group: Optional[dist.ProcessGroup],
                 world_size: int, wire_dtype=torch.float32,
                 bucket_cap_elems: int = DEFAULT_BUCKET_CAP_ELEMS, kernels=None,
                 exchange: str = "rccl", error_feedback: bool = False):
        self.params = list(params)
        self.k = kernels or default_kernels()
        self.device = self.params[0].device
        self.group, self.world_size = group, int(world_size)
        if exchange not in ("rccl", "a2a"):
            raise ValueError(f"exchange {exchange!r}: 'rccl' or 'a2a'")
        self.a2a = exchange == "a2a"
        if isinstance(wire_dtype, str) and wire_dtype != "fp4":
            raise ValueError(f"wire_dtype {wire_dtype!r}: a torch dtype or 'fp4'")
        self.q8 = wire_dtype == torch.int8
        self.fp4 = wire_dtype == "fp4"
        # a slot wire (int8, fp4): the bytes of one chunk's slot; None on the flat wires
        self.slot_bytes = SLOT_WIRES.get(wire_dtype)
        # slot wires only: carry what each quantiser rounds away into the next sync
        # (dl_gather_q8_ef, dl_q8_reduce_ef; dl_gather_fp4 / dl_fp4_reduce with a residual)
        self.error_feedback = bool(error_feedback)
        if self.error_feedback and self.slot_bytes is None:
            raise ValueError("error_feedback compensates the int8 / fp4 wire's quantiser; it "
                             "needs wire_dtype=torch.int8 or 'fp4'")
        if self.slot_bytes is not None and self.a2a:
            raise ValueError(f"the {'fp4' if self.fp4 else 'int8'} wire has its own rank-order "
                             "exchange; exchange='a2a' averages the fp32 grads")
        if dist.is_initialized() and self.world_size > 1:
            gs = dist.get_world_size(group)
            if gs != self.world_size:  # the collectives would reduce over the wrong ranks
                raise ValueError(f"GradSync(world_size={self.world_size}) on a process group "
                                 f"of {gs} ranks")
        # one replica: the all-reduce is the identity -- with no process group, or a group of
        # other ranks this replica does not average with (OuterSync._local's rule); a one-rank
        # group carries it (the single-rank RCCL transport test)
        self.local = self.world_size == 1 and (
            not dist.is_initialized() or dist.get_world_size(group) != 1)
        if self.a2a and wire_dtype != torch.float32:
            raise ValueError("GradSync(exchange='a2a') averages the fp32 grads")
        self.numels = [p.numel() for p in self.params]
        # a2a: buckets split into n equal 64-element-aligned shards
        balign = _lib.ALIGN_ELEMS * (self.world_size if self.a2a else 1)
        self.tree = self.k.tree(self.numels, self.device, bucket_cap_elems, balign)
        if self.slot_bytes is not None:
            self.wire = None
            self._alloc_slots()
        else:
            self.wire = torch.zeros(self.tree.total, dtype=wire_dtype, device=self.device)
        if self.a2a:
            n = self.world_size
            smax = max((hi - lo) // n for lo, hi in self.tree.bucket_ranges) if \
                self.tree.n_buckets else 0
            z = dict(dtype=torch.float32, device=self.device)
            # landing buffers and averaged shards, one per bucket in flight
            self.a2a_recv = [torch.zeros(n * smax, **z) for _ in range(2)]
            self.a2a_avg = [torch.zeros(smax, **z) for _ in range(2)]
        # own stream, joined back into the caller's (see OuterSync.stream)
        self.stream = torch.cuda.Stream(self.device) if self.device.type == "cuda" else None
        self.partials = None  # per-chunk Σ g² of sync(max_norm), created on first use

    def _alloc_slots(self) -> None:
        """OuterSync's slot plan: a region of n * m_b slots per bucket, zero at allocation (the
        padding slots are never encoded), landing and reduce buffers for two buckets in flight."""
        n, S = self.world_size, self.slot_bytes
        self.q8_plan, total, _owned, mmax = q8_slot_plan(self.tree.bucket_chunks, n)
        z = dict(dtype=torch.uint8, device=self.device)
        self.q_slots = torch.zeros(total * S, **z)
        self.q_recv = self.q_red = None
        if not self.local:
            self.q_recv = [torch.zeros(n * mmax * S, **z) for _ in range(2)]
            self.q_red = [torch.zeros(mmax * S, **z) for _ in range(2)]
        # error feedback: the encoder's residual in the packed layout, and at n > 1 the
        # residual of this peer's m_b re-quantised slots of every bucket
        self.q_residual = self.q_residual_red = None
        if self.error_feedback:
            f = dict(dtype=torch.float32, device=self.device)
            self.q_residual = torch.zeros(self.tree.total, **f)
            if n > 1:
                self.q_residual_red = [torch.zeros(m * _lib.CHUNK_ELEMS, **f)
                                       for _nch, m, _at, _rat in self.q8_plan]

    def q8_region(self, bucket: int) -> torch.Tensor:
        """The int8 / fp4 slots of one bucket (n * m slots, chunk order, zero padding at the
        end)."""
        _nch, m, at, _rat = self.q8_plan[bucket]
        S = self.slot_bytes
        return self.q_slots[at * S:(at + self.world_size * m) * S]

    def q8_ef_state(self) -> Optional[dict]:
        """{"encode": the encoder's residual, "reduce": [this peer's stage-2 residual per
        bucket]} as clones (the mirror's q8_ef_state); None when error feedback is off. The
        int8 and the fp4 wire keep the same arenas (fp32, the same shapes): one accessor pair."""
        if not self.error_feedback:
            return None
        return {"encode": self.q_residual.clone(),
                "reduce": [r.clone() for r in self.q_residual_red or []]}

    def load_q8_ef_state(self, state: Optional[dict]) -> None:
        """Copy a q8_ef_state() back (None: reset every residual to zero). A state that does
        not fit this exchange's buckets and peer count raises ValueError."""
        if not self.error_feedback:
            if state is None:
                return
            raise ValueError("this gradient sync runs without int8 error feedback")
        dst = self.q_residual_red or []
        if state is None:
            self.q_residual.zero_()
            for r in dst:
                r.zero_()
            return
        enc, red = state["encode"], list(state["reduce"])
        if tuple(enc.shape) != (self.tree.total,):
            raise ValueError(f"int8 error-feedback state: encode residual of {tuple(enc.shape)}, "
                             f"expected ({self.tree.total},)")
        if len(red) != len(dst) or any(tuple(a.shape) != tuple(d.shape)
                                       for a, d in zip(red, dst)):
            raise ValueError("the int8 error-feedback state does not match this exchange's "
                             "buckets and peer count")
        self.q_residual.copy_(enc)
        for d, a in zip(dst, red):
            d.copy_(a)

    def matches(self, params: Sequence[torch.Tensor]) -> bool:
        return len(params) == len(self.params) and all(
            a is b for a, b in zip(params, self.params))

    def sync(self, max_norm: Optional[float] = None) -> Optional[torch.Tensor]:
        """Average the gradients; with max_norm also clip them to it, as clip_grad_norm_ after
        the sync would, and return the total norm (a 0-dim fp32 tensor on the device; no host
        synchronisation). None: the sync alone, nothing returned."""
        clip = None
        if max_norm is not None:
            if self.partials is None:
                self.partials = torch.zeros(max(1, self.tree.n_chunks), dtype=torch.float64,
                                            device=self.device)
            # (norm, coefficient): a fresh pair per call, allocated on the caller's stream --
            # the caller keeps the norm
            clip = (float(max_norm), torch.empty(2, dtype=torch.float32, device=self.device))
        cur = None if self.stream is None else torch.cuda.current_stream(self.device)
        if cur is None or cur == self.stream:
            self._sync(clip)
        else:
            self.stream.wait_stream(cur)
            with torch.cuda.stream(self.stream):
                self._sync(clip)
            cur.wait_stream(self.stream)
        return None if clip is None else clip[1][0]

    def _unpack(self, b: int, divisor: int, clip) -> None:
        if clip is None:
            self.k.unpack_avg(self.tree, b, self.wire, divisor, SLOT_GRAD)
        else:
            self.k.unpack_avg_sumsq(self.tree, b, self.wire, divisor, SLOT_GRAD, self.partials)

    def _sync(self, clip=None) -> None:
        self._average(clip)
        if clip is not None:  # every bucket's partial sums are in: the norm, then one scaling
            max_norm, out2 = clip
            self.k.norm_finish(self.partials, max_norm, out2)
            self.k.scale_by(self.tree, _lib.ALL_BUCKETS, SLOT_GRAD, out2[1:])

    def _average(self, clip) -> None:
        grads = [p.grad for p in self.params]
        for i, g in enumerate(grads):
            if g.dtype != torch.float32 or not g.is_contiguous():
                raise TypeError(f"grad {i}: {g.dtype}, contiguous={g.is_contiguous()}; "
                                "the DP sync kernels take contiguous fp32 gradients")
        self.k.bind(self.tree, SLOT_GRAD, grads, self.device)

        def view(b):
            lo, hi = self.tree.bucket_ranges[b]
            return self.wire[lo:hi]

        # one replica (self.local): the all-reduce is the identity (the rebinding, gather and
        # /1 still run, so the path is exercised on a one-GPU machine)
        local = self.local
        if self.slot_bytes is not None:
            self._sync_slots(clip)
            return
        if self.a2a and not local:
            self._sync_a2a(clip)
            return
        pipelined_buckets(
            self.tree.n_buckets,
            lambda b: self.k.gather(self.tree, b, SLOT_GRAD, self.wire),
            lambda b: _Done() if local else dist.all_reduce(
                view(b), op=dist.ReduceOp.SUM, group=self.group, async_op=True),
            lambda b: self._unpack(b, self.world_size, clip),
        )

    def _sync_a2a(self, clip=None) -> None:
        """gather(b) -> all_to_all(b) | rank-order average(b) -> all_gather(b) | copy back(b),
        overlapped across buckets like OuterSync's sharded step."""
        n, nb = self.world_size, self.tree.n_buckets

        def shard(b):
            lo, hi = self.tree.bucket_ranges[b]
            return (hi - lo) // n

        def a2a(b):
            lo, hi = self.tree.bucket_ranges[b]
            self.k.gather(self.tree, b, SLOT_GRAD, self.wire)
            return dist.all_to_all_single(self.a2a_recv[b % 2][:n * shard(b)], self.wire[lo:hi],
                                          group=self.group, async_op=True)

        if nb == 0:
            return
        x, ag = [None] * nb, [None] * nb
        x[0] = a2a(0)
        for b in range(nb):
            if b + 1 < nb:
                x[b + 1] = a2a(b + 1)
            x[b].wait()
            s = shard(b)
            self.k.shard_reduce_avg(self.a2a_recv[b % 2][:n * s], n, self.a2a_avg[b % 2][:s])
            lo, hi = self.tree.bucket_ranges[b]
            ag[b] = dist.all_gather_into_tensor(self.wire[lo:hi], self.a2a_avg[b % 2][:s],
                                                group=self.group, async_op=True)
            if b >= 1:
                ag[b - 1].wait()
                self._unpack(b - 1, 1, clip)
        ag[nb - 1].wait()
        self._unpack(nb - 1, 1, clip)

    def _codec(self):
        """(encode(b), reduce(recv, n, m, divisor, residual, out), decode(b, partials)) of this
        slot wire; residual None: the call without error feedback."""
        k, tree = self.k, self.tree
        resid = self.q_residual  # None without error feedback
        if self.fp4:
            return (lambda b: k.gather_fp4(tree, b, SLOT_GRAD, resid, self.q8_region(b)),
                    k.fp4_reduce,
                    lambda b, p: k.unpack_avg_fp4(tree, b, self.q8_region(b), SLOT_GRAD, p))

        def encode(b):
            if resid is not None:
                k.gather_q8_ef(tree, b, SLOT_GRAD, resid, self.q8_region(b))
            else:
                k.gather_q8(tree, b, SLOT_GRAD, self.q8_region(b))

        def reduce(recv, n, m, divisor, residual, out):
            if residual is not None:
                k.q8_reduce_ef(recv, n, m, divisor, residual, out)
            else:
                k.q8_reduce(recv, n, m, divisor, out)

        return encode, reduce, lambda b, p: k.unpack_avg_q8(tree, b, self.q8_region(b),
                                                            SLOT_GRAD, p)

    def _sync_slots(self, clip=None) -> None:
        """encode(b) -> all_to_all(b) | reduce(b) -> all_gather(b) | decode(b) with the wire's
        three calls (_codec: gather_q8 / q8_reduce / unpack_avg_q8, or their fp4 twins),
        overlapped across buckets like _sync_a2a; the landing and reduce buffers alternate, so
        the bytes do not depend on the overlap."""
        n, nb, S = self.world_size, self.tree.n_buckets, self.slot_bytes
        partials = None if clip is None else self.partials
        encode, reduce, decode = self._codec()

        if self.local:
            # one replica: the average of one is its own re-quantised slots (error feedback:
            # only the encoder's residual -- re-quantising one peer's own slots is no second
            # lossy stage to compensate), so a one-GPU machine exercises the path
            for b in range(nb):
                region = self.q8_region(b)
                encode(b)
                reduce(region, 1, self.q8_plan[b][1], 1, None, region)
                decode(b, partials)
            return

        def a2a(b):
            m = self.q8_plan[b][1]
            encode(b)
            return dist.all_to_all_single(self.q_recv[b % 2][:n * m * S], self.q8_region(b),
                                          group=self.group, async_op=True)

        if nb == 0:
            return
        x, ag = [None] * nb, [None] * nb
        x[0] = a2a(0)
        for b in range(nb):
            if b + 1 < nb:
                x[b + 1] = a2a(b + 1)
            x[b].wait()
            m = self.q8_plan[b][1]
            recv, red = self.q_recv[b % 2][:n * m * S], self.q_red[b % 2][:m * S]
            resid = None if self.q_residual_red is None else self.q_residual_red[b]
            reduce(recv, n, m, n, resid, red)
            ag[b] = dist.all_gather_into_tensor(self.q8_region(b), red, group=self.group,
                                                async_op=True)
            if b >= 1:
                ag[b - 1].wait()
                decode(b - 1, partials)
        ag[nb - 1].wait()
        decode(nb - 1, partials)

    def close(self) -> None:
        self.tree.close()
