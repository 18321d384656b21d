"""Q8AdamWOracleKernels plus stand-ins for dl_delta_q8_ef and dl_q8_reduce_ef. TEST INFRASTRUCTURE.

Both are tests/q8_ef_restatement.py's chunk functions walked over the checker backend's chunk
table, so the engines' error-feedback orchestration runs on gloo CPU ranks and the HIP kernels
have a packed-layout reference. The residuals are updated in place, as on the device."""
import numpy as np

import q8_ef_restatement as ef
from oracle import oracle
from oracle_kernels import _np
from q8_adamw_oracle_kernels import Q8AdamWOracleKernels


class Q8EFOracleKernels(Q8AdamWOracleKernels):
    """Calls are logged as ("delta_q8_ef", bucket) and ("q8_reduce_ef", n_slots)."""

    def delta_q8_ef(self, tree, bucket, inner_slot, theta, residual, slots):
        self.calls.append(("delta_q8_ef", bucket))
        c0, c1 = self._chunk_range(tree, bucket)
        th, r, q = _np(theta), _np(residual), _np(slots)
        for c in range(c0, c1):
            seg, o, n, po = tree.chunks[c]
            inner = _np(tree.slots[inner_slot][seg])[o:o + n]
            j = (c - c0) * oracle.Q8_SLOT
            q[j:j + oracle.Q8_SLOT], r[po:po + n] = ef.encode_chunk(
                th[po:po + n].copy(), inner.copy(), r[po:po + n].copy())

    def q8_reduce_ef(self, recv, n_peers, n_slots, divisor, residual, out):
        self.calls.append(("q8_reduce_ef", n_slots))
        red, res = ef.reduce_slots(_np(recv).copy(), n_peers, n_slots, divisor,
                                   _np(residual).copy())
        _np(out)[:red.size] = red
        _np(residual)[:res.size] = res
