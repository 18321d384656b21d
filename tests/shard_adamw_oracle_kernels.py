"""AdamWOracleKernels plus a numpy stand-in for the two flat-shard AdamW kernels. TEST
INFRASTRUCTURE.

dl_shard_adamw and dl_shard_reduce_adamw restated with tests/adamw_restatement.py and the C
oracle's rank-order average (oracle.sum_avg) over the checker backend's CPU views, so the
mirrors' sharded / a2a AdamW step runs on gloo CPU ranks."""
import numpy as np
import torch

from adamw_oracle_kernels import AdamWOracleKernels
from adamw_restatement import adamw_elementwise
from oracle import oracle
from oracle_kernels import _np


class ShardAdamWOracleKernels(AdamWOracleKernels):
    """Calls are logged as (kernel name, shard elements) for the two shard kernels."""

    def _step(self, g, theta, exp_avg, exp_avg_sq, scalars):
        sc = tuple(np.float32(x) for x in scalars)  # the C-ABI's float arguments
        th, m, v = adamw_elementwise(_np(theta).copy(), _np(exp_avg).copy(),
                                     _np(exp_avg_sq).copy(), np.ascontiguousarray(g, np.float32),
                                     sc)
        _np(theta)[:] = th
        _np(exp_avg)[:] = m
        _np(exp_avg_sq)[:] = v

    def shard_adamw(self, wire, divisor, theta, exp_avg, exp_avg_sq, scalars):
        self.calls.append(("shard_adamw", theta.numel()))
        g = wire.float().numpy().copy()
        if divisor != 1:
            g = (g / np.float32(divisor)).astype(np.float32)
        self._step(g, theta, exp_avg, exp_avg_sq, scalars)

    def shard_reduce_adamw(self, slices, n_slices, theta, exp_avg, exp_avg_sq, scalars,
                           avg_out=None):
        """Σ over the n slices in rank order, /n (oracle/or_sum_avg), then the shard's AdamW."""
        self.calls.append(("shard_reduce_adamw", theta.numel()))
        assert slices.dtype == torch.float32
        L, s = theta.numel(), _np(slices)
        g = oracle.sum_avg([np.ascontiguousarray(s[q * L:(q + 1) * L]) for q in range(n_slices)])
        if avg_out is not None:
            _np(avg_out)[:] = g
        self._step(g, theta, exp_avg, exp_avg_sq, scalars)
