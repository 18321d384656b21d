"""ShardAdamWOracleKernels plus a numpy stand-in for dl_unpack_adamw_q8. TEST INFRASTRUCTURE.

Per chunk of the bucket: the averaged int8 slot dequantised by the C oracle (or_q8_deq, as
OracleKernels.unpack_sgd_q8 does), one step of tests/adamw_restatement.py on θ, exp_avg and
exp_avg_sq, then the inner write, so OuterAdamW's step after the int8 exchange runs on gloo CPU
ranks."""
import numpy as np

from adamw_restatement import adamw_elementwise
from oracle import oracle
from oracle_kernels import _np
from shard_adamw_oracle_kernels import ShardAdamWOracleKernels


class Q8AdamWOracleKernels(ShardAdamWOracleKernels):
    """Calls are logged as ("unpack_adamw_q8", bucket)."""

    def unpack_adamw_q8(self, tree, bucket, slots, theta, exp_avg, exp_avg_sq, scalars,
                        inner_slot):
        self.calls.append(("unpack_adamw_q8", bucket))
        sc = tuple(np.float32(x) for x in scalars)  # the C-ABI's float arguments
        c0, c1 = self._chunk_range(tree, bucket)
        q = _np(slots)
        for c in range(c0, c1):
            seg, o, n, po = tree.chunks[c]
            j = (c - c0) * oracle.Q8_SLOT
            g = np.empty(n, dtype=np.float32)
            oracle.load().or_q8_deq(oracle._u8(q[j:j + oracle.Q8_SLOT]), n, oracle._fp(g))
            th, m, v = adamw_elementwise(_np(theta)[po:po + n].copy(),
                                         _np(exp_avg)[po:po + n].copy(),
                                         _np(exp_avg_sq)[po:po + n].copy(), g, sc)
            _np(theta)[po:po + n] = th
            _np(exp_avg)[po:po + n] = m
            _np(exp_avg_sq)[po:po + n] = v
            if inner_slot >= 0:
                _np(tree.slots[inner_slot][seg])[o:o + n] = th
