"""The checker backends plus stand-ins for dl_gather_q8, dl_gather_q8_ef and dl_unpack_avg_q8.
TEST INFRASTRUCTURE.

Q8EFOracleKernels (the int8 codec, its reduces and error feedback) and ClipOracleKernels (the
gradient-norm kernels and the tree with n_chunks) in one backend, so GradSync's int8 exchange
runs on gloo CPU ranks and the three HIP kernels have a packed-layout reference:
  gather_q8       or_delta_q8 with a zero inner (x - (+0) = x bit for bit)
  gather_q8_ef    q8_ef_restatement.encode_chunk(g, 0, r)
  unpack_avg_q8   or_q8_deq into the destination; partials[c] = clip_restatement.chunk_sumsq
                  of the values stored
The residual is updated in place, as on the device."""
import numpy as np

import q8_ef_restatement as ef
from clip_oracle_kernels import ClipOracleKernels
from clip_restatement import chunk_sumsq
from oracle import oracle
from oracle_kernels import _np
from q8_ef_oracle_kernels import Q8EFOracleKernels

SLOT = oracle.Q8_SLOT


class GradSyncQ8OracleKernels(Q8EFOracleKernels, ClipOracleKernels):
    """Calls are logged as ("gather_q8" | "gather_q8_ef" | "unpack_avg_q8", bucket) and
    ("q8_reduce", n_slots), besides what the two parents log."""

    def __init__(self):
        ClipOracleKernels.__init__(self)  # calls, trees

    def gather_q8(self, tree, bucket, src_slot, slots):
        self.calls.append(("gather_q8", bucket))
        c0, c1 = self._chunk_range(tree, bucket)
        q = _np(slots)
        for c in range(c0, c1):
            seg, o, n, _po = tree.chunks[c]
            g = np.ascontiguousarray(_np(tree.slots[src_slot][seg])[o:o + n])
            j = (c - c0) * SLOT
            oracle.load().or_delta_q8(oracle._fp(g), oracle._fp(np.zeros(n, dtype=np.float32)),
                                      n, oracle._u8(q[j:j + SLOT]))

    def gather_q8_ef(self, tree, bucket, src_slot, residual, slots):
        self.calls.append(("gather_q8_ef", bucket))
        c0, c1 = self._chunk_range(tree, bucket)
        r, q = _np(residual), _np(slots)
        for c in range(c0, c1):
            seg, o, n, po = tree.chunks[c]
            g = _np(tree.slots[src_slot][seg])[o:o + n]
            j = (c - c0) * SLOT
            q[j:j + SLOT], r[po:po + n] = ef.encode_chunk(
                g.copy(), np.zeros(n, dtype=np.float32), r[po:po + n].copy())

    def q8_reduce(self, recv, n_peers, n_slots, divisor, out):
        self.calls.append(("q8_reduce", n_slots))
        super().q8_reduce(recv, n_peers, n_slots, divisor, out)

    def unpack_avg_q8(self, tree, bucket, slots, dst_slot, partials=None):
        self.calls.append(("unpack_avg_q8", bucket))
        c0, c1 = self._chunk_range(tree, bucket)
        q = _np(slots)
        for c in range(c0, c1):
            seg, o, n, _po = tree.chunks[c]
            j = (c - c0) * SLOT
            g = np.empty(n, dtype=np.float32)
            oracle.load().or_q8_deq(oracle._u8(np.ascontiguousarray(q[j:j + SLOT])), n,
                                    oracle._fp(g))
            _np(tree.slots[dst_slot][seg])[o:o + n] = g
            if partials is not None:
                _np(partials)[c] = chunk_sumsq(g)


NEW_METHODS = ("gather_q8", "gather_q8_ef", "unpack_avg_q8")
