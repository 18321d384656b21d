"""Q8EFOracleKernels plus stand-ins for the four fp4-wire calls. TEST INFRASTRUCTURE.

dl_delta_fp4 and dl_fp4_reduce are tests/fp4_restatement.py's chunk functions walked over the
checker backend's chunk table; dl_unpack_sgd_fp4 / dl_unpack_adamw_fp4 decode each slot with the
restatement and step with the C oracle's SGD / tests/adamw_restatement.py, as the int8 stand-ins
do. So the mirror's fp4 orchestration runs on gloo CPU ranks and the HIP kernels have a
packed-layout reference. Residuals are updated in place, as on the device."""
import numpy as np

import fp4_restatement as fp4
from adamw_restatement import adamw_elementwise
from oracle import oracle
from oracle_kernels import _np
from q8_ef_oracle_kernels import Q8EFOracleKernels

SLOT = fp4.SLOT


class Fp4OracleKernels(Q8EFOracleKernels):
    """Calls are logged as ("delta_fp4", bucket, ef), ("fp4_reduce", n_slots, ef),
    ("unpack_sgd_fp4", bucket) and ("unpack_adamw_fp4", bucket)."""

    def delta_fp4(self, tree, bucket, inner_slot, theta, residual, slots):
        self.calls.append(("delta_fp4", bucket, residual is not None))
        c0, c1 = self._chunk_range(tree, bucket)
        th, q = _np(theta), _np(slots)
        r = None if residual is None else _np(residual)
        for c in range(c0, c1):
            seg, o, n, po = tree.chunks[c]
            inner = _np(tree.slots[inner_slot][seg])[o:o + n]
            j = (c - c0) * SLOT
            q[j:j + SLOT], res = fp4.encode_chunk(th[po:po + n].copy(), inner.copy(),
                                                  None if r is None else r[po:po + n].copy())
            if r is not None:
                r[po:po + n] = res

    def fp4_reduce(self, recv, n_peers, n_slots, divisor, residual, out):
        self.calls.append(("fp4_reduce", n_slots, residual is not None))
        red, res = fp4.reduce_slots(_np(recv).copy(), n_peers, n_slots, divisor,
                                    None if residual is None else _np(residual).copy())
        _np(out)[:red.size] = red
        if residual is not None:
            _np(residual)[:res.size] = res

    def _fp4_chunks(self, tree, bucket, slots):
        c0, c1 = self._chunk_range(tree, bucket)
        q = _np(slots)
        for c in range(c0, c1):
            seg, o, n, po = tree.chunks[c]
            j = (c - c0) * SLOT
            yield seg, o, n, po, np.ascontiguousarray(fp4.decode_slot(q[j:j + SLOT], n))

    def unpack_sgd_fp4(self, tree, bucket, slots, theta, mom, lr, momentum, nesterov, first,
                       inner_slot):
        self.calls.append(("unpack_sgd_fp4", bucket))
        for seg, o, n, po, g in self._fp4_chunks(tree, bucket, slots):
            th = _np(theta)[po:po + n].copy()
            b = _np(mom)[po:po + n].copy() if mom is not None else None
            oracle.sgd(th, b, g, lr, momentum, nesterov, first)
            _np(theta)[po:po + n] = th
            if mom is not None:
                _np(mom)[po:po + n] = b
            if inner_slot >= 0:
                _np(tree.slots[inner_slot][seg])[o:o + n] = th

    def unpack_adamw_fp4(self, tree, bucket, slots, theta, exp_avg, exp_avg_sq, scalars,
                         inner_slot):
        self.calls.append(("unpack_adamw_fp4", bucket))
        sc = tuple(np.float32(x) for x in scalars)  # the C-ABI's float arguments
        for seg, o, n, po, g in self._fp4_chunks(tree, bucket, slots):
            th, m, v = adamw_elementwise(_np(theta)[po:po + n].copy(),
                                         _np(exp_avg)[po:po + n].copy(),
                                         _np(exp_avg_sq)[po:po + n].copy(), g, sc)
            _np(theta)[po:po + n] = th
            _np(exp_avg)[po:po + n] = m
            _np(exp_avg_sq)[po:po + n] = v
            if inner_slot >= 0:
                _np(tree.slots[inner_slot][seg])[o:o + n] = th
