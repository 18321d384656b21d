"""Streaming DiLoCo (Douillard et al., 2025) on the replicated exchange: the tree syncs in P
fragments at staggered inner steps, each fragment's exchange runs while τ more inner steps are
computed, and the inner model is MERGED with the new θ_outer instead of overwritten.

    fragment p begins at every inner step t with t % H == ((p + 1) * (H // P)) % H:
        wire[b] = θ_outer[b] - inner[b]; async all-reduce of bucket b     (per bucket of p)
    and finishes τ steps later:
        wait; g = wire/n; Nesterov SGD on θ_outer[b];
        inner[b] = α·inner[b] + (1 - α)·θ_outer[b]         (dl_unpack_sgd_merge, one pass)

Each fragment still syncs once per H inner steps, but only about 1/P of the bytes is on the wire
at a time, and the inner loop does not wait for the exchange. A bucket's region of the wire holds
its exchange while it is in flight: τ < H means a bucket has at most one open, so the engine
needs no buffers beyond OuterSync's. Inner steps between a begin and its finish touch neither
the wire nor θ_outer.

With P = 1, τ = 0 and α = 0 the schedule and the arithmetic are OuterSync(shard=False).step()
at every H-th inner step.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import torch

from .outer import OuterSync, _Done
from .plan import SLOT_INNER

PATTERNS = ("strided", "sequential")


def _check_schedule(sync_every: int, fragments: int, delay: int) -> int:
    H, P, tau = int(sync_every), int(fragments), int(delay)
    if H < 1 or P < 1:
        raise ValueError(f"sync_every {sync_every} and fragments {fragments} must be >= 1")
    if H % P != 0:
        raise ValueError(f"sync_every {H} is not a multiple of fragments {P}")
    if not 0 <= tau < H:
        raise ValueError(f"delay {delay}: 0 <= delay < sync_every ({H}), so that a fragment's "
                         "exchange is finished before its next one begins")
    return H // P


def fragment_events(t: int, sync_every: int, fragments: int, delay: int) -> Tuple[list, list]:
    """(finish, begin) after inner step t >= 1: the fragments whose outer step is applied now,
    in the order they began, and the fragment (at most one) whose exchange begins now. Fragment p
    begins at every t with t % H == ((p + 1) * S) % H, S = H // P, and finishes `delay` steps
    after it began. A function of t alone, so every rank issues the same collectives in the same
    order."""
    S = _check_schedule(sync_every, fragments, delay)
    H, P, tau = int(sync_every), int(fragments), int(delay)
    if t < 1:
        raise ValueError(f"t {t}: the number of inner steps done, >= 1")
    begin = [p for p in range(P) if t % H == ((p + 1) * S) % H]
    tb = t - tau  # the step at which a fragment due now began
    finish = [p for p in range(P) if tb >= 1 and tb % H == ((p + 1) * S) % H]
    return finish, begin


def split_buckets(n_buckets: int, fragments: int, pattern: str) -> List[List[int]]:
    """The buckets of each fragment. strided: b % P == p; sequential: P contiguous runs whose
    sizes differ by at most one (the longer ones first)."""
    if pattern not in PATTERNS:
        raise ValueError(f"pattern {pattern!r}: 'strided' or 'sequential'")
    P = int(fragments)
    if n_buckets < P:
        raise ValueError(f"{n_buckets} buckets cannot make {P} fragments: lower "
                         "bucket_cap_elems (a fragment is a set of buckets)")
    if pattern == "strided":
        return [list(range(p, n_buckets, P)) for p in range(P)]
    q, r = divmod(n_buckets, P)
    out, at = [], 0
    for p in range(P):
        n = q + (1 if p < r else 0)
        out.append(list(range(at, at + n)))
        at += n
    return out


class StreamingOuterSync(OuterSync):
    """OuterSync whose outer step is streamed: call after_inner_step() once after every inner
    optimizer step, on the stream that step ran on; flush() at the end of training and before a
    checkpoint."""

    def __init__(self, params, *, sync_every: int, fragments: int = 1, delay: int = 0,
                 alpha: float = 0.0, pattern: str = "strided", **outer_sync_kwargs):
        _check_schedule(sync_every, fragments, delay)
        if not 0.0 <= float(alpha) < 1.0:  # a NaN fails the comparison too
            raise ValueError(f"alpha {alpha}: 0 <= alpha < 1")
        if pattern not in PATTERNS:
            raise ValueError(f"pattern {pattern!r}: 'strided' or 'sequential'")
        kw = dict(outer_sync_kwargs)
        if kw.get("shard"):
            raise ValueError("StreamingOuterSync runs on the replicated exchange: shard=True is "
                             "not streamed")
        if kw.get("exchange", "rccl") != "rccl":
            raise ValueError(f"StreamingOuterSync runs on the replicated all-reduce: exchange="
                             f"{kw['exchange']!r} is not streamed")
        if kw.get("wire_dtype", torch.float32) == torch.int8:
            raise ValueError("StreamingOuterSync exchanges the fp32 or bf16 wire: "
                             "wire_dtype=torch.int8 is not streamed")
        if kw.get("error_feedback"):
            raise ValueError("StreamingOuterSync has no int8 wire: error_feedback=True is not "
                             "streamed")
        kw["shard"] = False
        # the events run on the caller's stream, where the inner step ran
        kw.setdefault("side_stream", False)
        super().__init__(params, **kw)
        self.sync_every, self.fragments = int(sync_every), int(fragments)
        self.delay, self.alpha, self.pattern = int(delay), float(alpha), pattern
        try:
            self.fragment_buckets = split_buckets(self.tree.n_buckets, self.fragments, pattern)
        except ValueError:
            self.tree.close()
            raise
        self.inner_steps = 0
        # first steps are per bucket: a bucket's momentum is created by its own first finish
        self.bucket_steps = [0] * self.tree.n_buckets
        self._works: Dict[int, list] = {}  # fragment -> [(bucket, handle)], in begin order

    @property
    def in_flight(self) -> List[int]:
        """The fragments begun and not finished, in begin order."""
        return list(self._works)

    def _begin(self, p: int) -> None:
        works = []
        for b in self.fragment_buckets[p]:
            self.pseudo_gradient(b)
            works.append((b, _Done() if self._local() else self.all_reduce(b, async_op=True)))
        self._works[p] = works

    def _finish(self, p: int) -> None:
        for b, work in self._works.pop(p):
            work.wait()
            self.k.unpack_sgd_merge(self.tree, b, self.wire, self.world_size, self.theta,
                                    self.mom, self.lr, self.momentum, self.nesterov,
                                    self.bucket_steps[b] == 0, SLOT_INNER, self.alpha)
            self.bucket_steps[b] += 1
        self.steps_done = min(self.bucket_steps)

    def after_inner_step(self) -> None:
        """Count one inner step; apply the outer step of the fragments due now (merging it into
        the inner parameters), then begin the exchange of the fragment that starts now. With
        delay 0 that fragment finishes in the same call."""
        self.inner_steps += 1
        finish, begin = fragment_events(self.inner_steps, self.sync_every, self.fragments,
                                        self.delay)
        if not finish and not begin:
            return
        self.k.bind(self.tree, SLOT_INNER, self.params, self.device)
        self._step_bound = True
        try:
            for p in finish:
                if p in self._works:  # not one that flush() finished early
                    self._finish(p)
            for p in begin:
                self._begin(p)
            if self.delay == 0:
                for p in begin:
                    self._finish(p)
        finally:
            self._step_bound = False

    def flush(self) -> None:
        """Finish every exchange in flight now, in begin order."""
        if not self._works:
            return
        self.k.bind(self.tree, SLOT_INNER, self.params, self.device)
        for p in list(self._works):
            self._finish(p)

    def step(self, pipeline=None) -> None:
        raise RuntimeError("StreamingOuterSync has no blocking step(): call after_inner_step() "
                           "after every inner optimizer step (and flush() at the end)")

    # ---- checkpoint / resume -----------------------------------------------------------------
    def state_dict(self) -> dict:
        if self._works:
            raise RuntimeError(f"fragments {self.in_flight} are in flight: call flush() before "
                               "state_dict()")
        self.steps_done = min(self.bucket_steps)
        state = super().state_dict()
        state.update(bucket_steps=list(self.bucket_steps), inner_steps=self.inner_steps,
                     sync_every=self.sync_every, fragments=self.fragments, delay=self.delay,
                     alpha=self.alpha)
        return state

    def load_state_dict(self, state: dict, write_inner: bool = False) -> None:
        """Restore a state_dict() of an engine with this bucket layout. After a merge the inner
        parameters are not θ_outer, so they are the inner model's own checkpoint: write_inner
        defaults to False here."""
        steps = [int(s) for s in state["bucket_steps"]]
        if len(steps) != self.tree.n_buckets:
            raise ValueError(f"state_dict has {len(steps)} buckets, this engine "
                             f"{self.tree.n_buckets}: bucket_steps follow the bucket layout")
        if self._works:
            raise RuntimeError(f"fragments {self.in_flight} are in flight: call flush() first")
        H, P, tau = int(state["sync_every"]), int(state["fragments"]), int(state["delay"])
        alpha = float(state["alpha"])
        _check_schedule(H, P, tau)
        if not 0.0 <= alpha < 1.0:
            raise ValueError(f"alpha {alpha}: 0 <= alpha < 1")
        self.fragment_buckets = split_buckets(self.tree.n_buckets, P, self.pattern)
        self.sync_every, self.fragments, self.delay, self.alpha = H, P, tau, alpha
        # the momentum of a bucket exists once that bucket has stepped, whatever min() says
        base = dict(state, steps=max(steps))
        super().load_state_dict(base, write_inner=write_inner)
        self.bucket_steps = steps
        self.steps_done = min(steps)
        self.inner_steps = int(state["inner_steps"])
