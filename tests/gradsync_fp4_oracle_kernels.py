"""The checker backends plus stand-ins for dl_gather_fp4 and dl_unpack_avg_fp4.
TEST INFRASTRUCTURE.

Fp4OracleKernels (the fp4 codec, its reduce and error feedback) and ClipOracleKernels (the
gradient-norm kernels and the tree with n_chunks) in one backend, so GradSync's fp4 exchange runs
on gloo CPU ranks and the two HIP kernels have a packed-layout reference:
  gather_fp4       fp4_restatement.encode_chunk(g, 0, r)   (x - (+0) = x bit for bit)
  unpack_avg_fp4   fp4_restatement.decode_slot into the destination; partials[c] =
                   clip_restatement.chunk_sumsq of the values stored
The residual is updated in place, as on the device."""
import numpy as np

import fp4_restatement as fp4
from clip_oracle_kernels import ClipOracleKernels
from clip_restatement import chunk_sumsq
from fp4_oracle_kernels import Fp4OracleKernels
from oracle_kernels import _np

SLOT = fp4.SLOT


class GradFp4StandIns:
    """The two stand-ins, for any checker backend with a chunk table and a call log. Calls are
    logged as ("gather_fp4", bucket, ef) and ("unpack_avg_fp4", bucket, partials given)."""

    def gather_fp4(self, tree, bucket, src_slot, residual, slots):
        self.calls.append(("gather_fp4", bucket, residual is not None))
        c0, c1 = self._chunk_range(tree, bucket)
        q = _np(slots)
        r = None if residual is None else _np(residual)
        for c in range(c0, c1):
            seg, o, n, po = tree.chunks[c]
            g = _np(tree.slots[src_slot][seg])[o:o + n]
            j = (c - c0) * SLOT
            q[j:j + SLOT], res = fp4.encode_chunk(g.copy(), np.zeros(n, dtype=np.float32),
                                                  None if r is None else r[po:po + n].copy())
            if r is not None:
                r[po:po + n] = res

    def unpack_avg_fp4(self, tree, bucket, slots, dst_slot, partials=None):
        self.calls.append(("unpack_avg_fp4", bucket, partials is not None))
        c0, c1 = self._chunk_range(tree, bucket)
        q = _np(slots)
        for c in range(c0, c1):
            seg, o, n, _po = tree.chunks[c]
            j = (c - c0) * SLOT
            g = np.ascontiguousarray(fp4.decode_slot(q[j:j + SLOT], n))
            _np(tree.slots[dst_slot][seg])[o:o + n] = g
            if partials is not None:
                _np(partials)[c] = chunk_sumsq(g)


class GradSyncFp4OracleKernels(GradFp4StandIns, Fp4OracleKernels, ClipOracleKernels):
    """Besides the stand-ins' log: ("fp4_reduce", n_slots, ef) and what the two parents log."""

    def __init__(self):
        ClipOracleKernels.__init__(self)  # calls, trees


NEW_METHODS = ("gather_fp4", "unpack_avg_fp4")
