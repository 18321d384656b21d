"""OracleKernels plus a numpy stand-in for the four gradient-norm kernels. TEST INFRASTRUCTURE.

dl_grad_sumsq, dl_unpack_avg_sumsq, dl_norm_finish and dl_scale_by restated with
tests/clip_restatement.py over the checker backend's CPU tensors, so GradSync.sync(max_norm),
DPSync and utils.clip_grad_norm_ run their orchestration without a GPU."""
import torch

from clip_restatement import chunk_sumsq, finish, scaled
from oracle_kernels import CpuTree, OracleKernels, _np


class ClipCpuTree(CpuTree):
    def __init__(self, numels, cap, bucket_align=64):
        super().__init__(numels, cap, bucket_align)
        self.n_chunks = len(self.chunks)
        self.closed = False

    def close(self):
        self.closed = True


class ClipOracleKernels(OracleKernels):
    def __init__(self):
        self.calls = []  # (kernel name, bucket) in launch order
        self.trees = []  # every tree handed out, in order

    def tree(self, numels, device, cap_elems=64 << 20, bucket_align=64):
        t = ClipCpuTree(numels, cap_elems, bucket_align)
        self.trees.append(t)
        return t

    def unpack_avg(self, tree, bucket, wire, divisor, dst_slot, dst_packed=None):
        self.calls.append(("unpack_avg", bucket))
        super().unpack_avg(tree, bucket, wire, divisor, dst_slot, dst_packed)

    def _sumsq(self, tree, bucket, chunk_values, partials):
        c0, c1 = self._chunk_range(tree, bucket)
        p = _np(partials)
        for c in range(c0, c1):
            p[c] = chunk_sumsq(chunk_values(*tree.chunks[c]))

    def grad_sumsq(self, tree, bucket, src_slot, partials):
        self.calls.append(("grad_sumsq", bucket))
        self._sumsq(tree, bucket,
                    lambda seg, o, n, po: _np(tree.slots[src_slot][seg])[o:o + n], partials)

    def unpack_avg_sumsq(self, tree, bucket, wire, divisor, dst_slot, partials, dst_packed=None):
        # one pass on the device; restated as the pair it is bit-identical to
        self.calls.append(("unpack_avg_sumsq", bucket))
        super().unpack_avg(tree, bucket, wire, divisor, dst_slot, dst_packed)
        if dst_slot >= 0:
            self._sumsq(tree, bucket,
                        lambda seg, o, n, po: _np(tree.slots[dst_slot][seg])[o:o + n], partials)
        else:
            self._sumsq(tree, bucket, lambda seg, o, n, po: _np(dst_packed)[po:po + n], partials)

    def norm_finish(self, partials, max_norm, out2):
        self.calls.append(("norm_finish", None))
        norm, coef = finish(_np(partials), max_norm)
        out2[0], out2[1] = float(norm), float(coef)

    def scale_by(self, tree, bucket, slot, coef):
        self.calls.append(("scale_by", bucket))
        k = _np(coef)[0]
        for i in tree.segs(bucket):
            g = _np(tree.slots[slot][i])
            g[:] = scaled(g, k)


NEW_METHODS = ("grad_sumsq", "unpack_avg_sumsq", "norm_finish", "scale_by")


def as_params(arrays):
    """CPU parameters whose .grad hold copies of the given fp32 arrays."""
    ps = []
    for a in arrays:
        p = torch.nn.Parameter(torch.zeros(a.size))
        p.grad = torch.from_numpy(a.copy())
        ps.append(p)
    return ps
