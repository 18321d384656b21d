"""OracleKernels plus a numpy stand-in for the two AdamW kernels. TEST INFRASTRUCTURE.

dl_unpack_adamw and dl_delta_pack_adamw restated with tests/adamw_restatement.py over the
checker backend's packed CPU buffers, so OuterAdamW and the mirrors' adamw_step run on CPU."""
import numpy as np

from adamw_restatement import adamw_elementwise
from oracle_kernels import OracleKernels, _np


class AdamWOracleKernels(OracleKernels):
    def __init__(self):
        self.calls = []  # (kernel name, bucket) in launch order

    def unpack_adamw(self, tree, bucket, wire, divisor, theta, exp_avg, exp_avg_sq, scalars,
                     inner_slot):
        self.calls.append(("unpack_adamw", bucket))
        self._adamw(tree, bucket, wire, divisor, theta, exp_avg, exp_avg_sq, scalars, inner_slot)

    def _adamw(self, tree, bucket, wire, divisor, theta, exp_avg, exp_avg_sq, scalars, inner_slot):
        sc = tuple(np.float32(x) for x in scalars)  # the C-ABI's float arguments
        for i in tree.segs(bucket):
            g = self._rd(tree, wire, i)
            if divisor != 1:
                g = (g / np.float32(divisor)).astype(np.float32)
            th, m, v = adamw_elementwise(self._seg(tree, theta, i).copy(),
                                         self._seg(tree, exp_avg, i).copy(),
                                         self._seg(tree, exp_avg_sq, i).copy(), g, sc)
            self._seg(tree, theta, i)[:] = th
            self._seg(tree, exp_avg, i)[:] = m
            self._seg(tree, exp_avg_sq, i)[:] = v
            if inner_slot >= 0:
                _np(tree.slots[inner_slot][i])[:] = th

    def delta_pack_adamw(self, tree, bucket, inner_slot, theta, wire, exp_avg, exp_avg_sq,
                         scalars):
        # one pass on the device; restated as the pair it is bit-identical to
        self.calls.append(("delta_pack_adamw", bucket))
        self.delta_pack(tree, bucket, inner_slot, theta, wire)
        self._adamw(tree, bucket, wire, 1, theta, exp_avg, exp_avg_sq, scalars, inner_slot)
