"""ClipOracleKernels plus a numpy stand-in for dl_adamw_step. TEST INFRASTRUCTURE.

The inner AdamW step restated with tests/adamw_restatement.py over the checker backend's CPU
tensors (θ and g per tensor in bound slots, exp_avg and exp_avg_sq packed), so optim.InnerAdamW
runs its orchestration without a GPU. A coefficient multiplies the gradient in fp32 first, one
rounding, as the kernel does; the gradients themselves are only read."""
import numpy as np

from adamw_restatement import F, adamw_elementwise
from clip_oracle_kernels import ClipOracleKernels
from oracle_kernels import _np


class InnerAdamWOracleKernels(ClipOracleKernels):
    def __init__(self):
        super().__init__()
        self.coefs = []  # per adamw_step call: None, or the coefficient it was handed

    def adamw_step(self, tree, bucket, param_slot, grad_slot, exp_avg, exp_avg_sq, scalars,
                   coef=None):
        self.calls.append(("adamw_step", bucket))
        k = None if coef is None else F(_np(coef)[0])
        self.coefs.append(k)
        sc = tuple(F(x) for x in scalars)  # the C-ABI's float arguments
        for i in tree.segs(bucket):
            th = _np(tree.slots[param_slot][i])
            g = _np(tree.slots[grad_slot][i]).copy()
            if k is not None:
                with np.errstate(all="ignore"):
                    g = (g * k).astype(F)
            m, v = self._seg(tree, exp_avg, i), self._seg(tree, exp_avg_sq, i)
            th[:], m[:], v[:] = adamw_elementwise(th.copy(), m.copy(), v.copy(), g, sc)
