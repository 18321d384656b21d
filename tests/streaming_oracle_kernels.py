"""OracleKernels plus stand-ins for the two merging kernels. TEST INFRASTRUCTURE.

dl_unpack_sgd_merge / dl_unpack_adamw_merge restated as the header states them: the existing
unpack_sgd / unpack_adamw arithmetic (θ, the state; inner <- θ), then inner <- merge(x, θ, alpha)
with x the inner values taken before the call (tests/streaming_restatement.merge). alpha 0 is the
non-merging call. So StreamingOuterSync runs on CPU tensors and over gloo."""
from adamw_oracle_kernels import AdamWOracleKernels
from oracle_kernels import _np
from streaming_restatement import merge


class MergeStandIns:
    def _merged(self, tree, bucket, inner_slot, alpha, step):
        assert inner_slot >= 0 and 0.0 <= alpha < 1.0
        segs = list(tree.segs(bucket))
        x = {i: _np(tree.slots[inner_slot][i]).copy() for i in segs}
        step()  # leaves inner = θ
        if alpha != 0:
            for i in segs:
                inner = _np(tree.slots[inner_slot][i])
                inner[:] = merge(x[i], inner.copy(), alpha)

    def unpack_sgd_merge(self, tree, bucket, wire, divisor, theta, mom, lr, momentum, nesterov,
                         first, inner_slot, alpha):
        self._merged(tree, bucket, inner_slot, alpha, lambda: self.unpack_sgd(
            tree, bucket, wire, divisor, theta, mom, lr, momentum, nesterov, first, inner_slot))

    def unpack_adamw_merge(self, tree, bucket, wire, divisor, theta, exp_avg, exp_avg_sq, scalars,
                           inner_slot, alpha):
        self._merged(tree, bucket, inner_slot, alpha, lambda: self._adamw(
            tree, bucket, wire, divisor, theta, exp_avg, exp_avg_sq, scalars, inner_slot))


class StreamingOracleKernels(MergeStandIns, AdamWOracleKernels):
    pass
