"""Every kernel's write footprint on the GPU, with non-zero sentinels (tests/footprint.py).

One test per kernel (and wire). Each runs its cases on the 19-chunk ragged tree under both
sentinel patterns, with the per-tensor storage at 0, 1 and mixed 0-3 elements off a 16-B boundary
(every pair of placements where a kernel binds two slots), whole-tree and bucket by bucket, and at
grid caps 0, 1, 2 and 5 (DL_TUNE_AUTO flags: cap 1 makes one workgroup walk all the chunks and
reuse its LDS for each), two or more consecutive calls per configuration. After every launch
every byte of every buffer -- outputs, inputs, padding, guard bands, the other buckets -- must
equal the CPU checker backend's, which tests/test_footprint_cpu.py shows to stay inside the
footprint itself. Nothing here is a tolerance: the comparison is bit for bit."""
import pytest
import torch

import footprint as fp
from diloco_amd.kernels import HipKernels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = HipKernels()


def _tree_rows():
    for name, (cases, wires) in fp.TREE_ROWS.items():
        for w in wires or (None,):
            yield pytest.param(cases, w, id=name + (f"-{w}" if w else ""))


@pytest.mark.parametrize("cases, wire", _tree_rows())
def test_tree_walker_footprint(cases, wire):
    assert torch.cuda.is_available()
    for case in cases(wire) if wire else cases():
        fp.run_case(case, K, DEV, grids=fp.GRIDS)


@pytest.mark.parametrize("row", list(fp.FLAT_ROWS))
def test_flat_kernel_footprint(row):
    """The flat kernels: guard bands before and after every buffer, every size and slice count
    of the row; the inputs (wire, slices, recv unless aliased) are only read."""
    for case in fp.FLAT_ROWS[row]():
        fp.run_flat_case(case, K, DEV)
