"""Streaming DiLoCo restated in numpy: the merge, the schedule and a simulator of n replicas.
TEST INFRASTRUCTURE.

The merge is the contract of dl_unpack_sgd_merge / dl_unpack_adamw_merge (include/diloco_hip.h):

    inner = fma(alpha, x - th, th)        x - th one rounded fp32 subtract, then ONE fma

with tests/adamw_restatement.fmaf as the fma (pinned against libm in tests/test_streaming_cpu.py).

StreamSim restates diloco_amd/streaming.py's engine literally over lists of flat fp32 arrays, with
no torch op in the arithmetic and none of the engine's code: its own schedule, its own fragment
split, the delta as one fp32 subtract (a bf16 wire rounds it), the sum over ranks in rank order
(a bf16 wire rounds every partial sum, the collective's bf16 SUM as tests/expect.
expected_bf16_allreduce has it), an IEEE division by n (none at n = 1), the SGD of oracle.sgd,
then the merge, with first steps per bucket.

The inner step between two calls is a stand-in, the same here and in the runs that are compared:
after inner step t, tensor i of rank r has moved by u(seed(r, t), i, ·)·1e-2, u the counter-based
generator of diloco_amd.synth."""
import numpy as np

from adamw_restatement import F, bf16_round, fmaf
from diloco_amd import synth
from diloco_amd.plan import plan_tables
from oracle import oracle

STEP_SCALE = 1e-2


def merge(x, th, alpha):
    """alpha·x + (1 - alpha)·th as the kernels compute it."""
    x, th = np.asarray(x, F), np.asarray(th, F)
    with np.errstate(all="ignore"):
        return fmaf(np.asarray(alpha, F), x - th, th)


def step_seed(rank, t):
    return 500000 + 1000 * t + rank


def perturbation(rank, t, i, n):
    """What the stand-in inner step t adds to tensor i (n elements) of rank `rank`."""
    return synth.uniform(step_seed(rank, t), i, n) * F(STEP_SCALE)


def inner_step(inner, rank, t):
    """The stand-in inner step on a list of flat fp32 arrays, in place."""
    for i, x in enumerate(inner):
        x += perturbation(rank, t, i, x.size)


def bucket_segments(numels, cap):
    """The tensors of every bucket, by the planner's rule."""
    _seg, bnd = plan_tables([int(n) for n in numels], cap)
    return [list(range(int(bnd[b]), int(bnd[b + 1]))) for b in range(len(bnd) - 1)]


def fragments_of(n_buckets, P, pattern):
    if pattern == "strided":
        return [[b for b in range(n_buckets) if b % P == p] for p in range(P)]
    assert pattern == "sequential"
    sizes = [n_buckets // P + (1 if p < n_buckets % P else 0) for p in range(P)]
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    return [list(range(starts[p], starts[p + 1])) for p in range(P)]


class StreamSim:
    def __init__(self, theta0, n, H, P, tau, alpha, cap, pattern="strided", wire="f32",
                 lr=0.7, momentum=0.9, nesterov=True):
        assert H % P == 0 and 0 <= tau < H
        self.theta = [np.array(t, F).reshape(-1) for t in theta0]
        self.mom = [np.zeros_like(t) for t in self.theta]
        self.wire = [np.zeros_like(t) for t in self.theta]  # fp32 values (bf16: exact in bf16)
        self.inner = [[t.copy() for t in self.theta] for _ in range(n)]
        self.n, self.H, self.P, self.tau, self.alpha = n, H, P, tau, alpha
        self.bf16 = wire == "bf16"
        self.lr, self.momentum, self.nesterov = lr, momentum, nesterov
        self.buckets = bucket_segments([t.size for t in self.theta], cap)
        self.frags = fragments_of(len(self.buckets), P, pattern)
        self.bucket_steps = [0] * len(self.buckets)
        self.t = 0
        self.open = {}  # fragment -> the step it began at, in begin order

    def inner_steps(self):
        """One stand-in inner step on every rank."""
        self.t += 1
        for r in range(self.n):
            inner_step(self.inner[r], r, self.t)

    def _begin(self, p):
        for b in self.frags[p]:
            for i in self.buckets[b]:
                acc = None
                for r in range(self.n):
                    d = self.theta[i] - self.inner[r][i]
                    if self.bf16:
                        d = bf16_round(d)
                    acc = d if acc is None else acc + d
                    if self.bf16 and r > 0:
                        acc = bf16_round(acc)
                self.wire[i] = acc
        self.open[p] = self.t

    def _finish(self, p):
        del self.open[p]
        for b in self.frags[p]:
            first = self.bucket_steps[b] == 0
            for i in self.buckets[b]:
                g = self.wire[i] if self.n == 1 else (self.wire[i] / F(self.n)).astype(F)
                if g.size:
                    oracle.sgd(self.theta[i], self.mom[i] if self.momentum else None,
                               np.ascontiguousarray(g), self.lr, self.momentum, self.nesterov,
                               first)
                for r in range(self.n):
                    self.inner[r][i] = (self.theta[i].copy() if self.alpha == 0 else
                                        merge(self.inner[r][i], self.theta[i], self.alpha))
            self.bucket_steps[b] += 1

    def after_inner_step(self):
        S = self.H // self.P
        for p in [q for q, t0 in self.open.items() if t0 + self.tau == self.t]:
            self._finish(p)
        for p in range(self.P):
            if self.t % self.H == ((p + 1) * S) % self.H:
                self._begin(p)
                if self.tau == 0:
                    self._finish(p)

    def flush(self):
        for p in list(self.open):
            self._finish(p)

    def flat(self, what, rank=0):
        x = self.inner[rank] if what == "inner" else getattr(self, what)
        return np.concatenate([np.asarray(t, F).reshape(-1) for t in x])
