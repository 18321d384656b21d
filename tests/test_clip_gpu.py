"""Gradient-norm clipping on the GPU: dl_grad_sumsq / dl_unpack_avg_sumsq / dl_norm_finish /
dl_scale_by against the numpy restatement of their summation order (tests/clip_restatement.py)
bit for bit, against torch in fp64 within the derived bound, and the Python surface
(utils.clip_grad_norm_, GradSync.sync(max_norm)) against torch's own call."""
import os
import socket
import sys
import tempfile

import numpy as np
import pytest
import torch

import clip_restatement as cr
from conftest import PKG, REPO
from diloco_amd import _lib, utils
from diloco_amd.gradsync import GradSync
from diloco_amd.kernels import HipKernels
from diloco_amd.plan import SLOT_AUX, SLOT_GRAD, PackedTree

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = _lib.ALL_BUCKETS
# 257 chunks in the last tensor: the finish kernel's stride loop runs a second round
NUMELS = [1, 3, 4, 63, 4095, 4096, 4097, 8197, 4096 * 256 + 7]
CAP = 8192  # elements per bucket: several buckets, the large tensor in one of its own
K = HipKernels()


def _values(seed=11, numels=NUMELS, scale=1.0):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(n) * scale).astype(np.float32) for n in numels]


def _on_device(vals, misaligned=False):
    """Device copies; misaligned: each a view one element (4 B) past a 16-B boundary."""
    out = []
    for v in vals:
        if misaligned:
            buf = torch.empty(v.size + 8, dtype=torch.float32, device=DEV)
            t = buf[1:1 + v.size]
            assert t.data_ptr() % 16 == 4
        else:
            t = torch.empty(v.size, dtype=torch.float32, device=DEV)
            assert t.data_ptr() % 16 == 0
        t.copy_(torch.from_numpy(v))
        out.append(t)
    return out


def _params(vals, misaligned=False):
    ps = []
    for g in _on_device(vals, misaligned):
        p = torch.nn.Parameter(torch.zeros(g.numel(), device=DEV))
        p.grad = g
        ps.append(p)
    return ps


def _bits(ts):
    return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in ts]).tobytes()


@pytest.fixture(scope="module")
def ref():
    """The shared values and their restated partial sums and norm; never modified."""
    vals = _values()
    parts = cr.tree_partials(vals)
    norm, _ = cr.finish(parts, 1.0)
    return dict(vals=vals, parts=parts, norm=norm)


@pytest.fixture
def tree():
    t = PackedTree(NUMELS, CAP)
    assert t.n_buckets >= 3 and t.n_chunks == 1 + 1 + 1 + 1 + 1 + 1 + 2 + 3 + 257
    yield t
    t.close()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _finish(partials, max_norm):
    out2 = torch.full((2,), float("nan"), device=DEV)
    K.norm_finish(partials, max_norm, out2)
    return out2


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("launch", ["all", "buckets", "max_blocks_3"])
def test_norm_matches_the_restatement_bit_for_bit(ref, tree, misaligned, launch):
    grads = _on_device(ref["vals"], misaligned)
    tree.bind(SLOT_GRAD, grads, _stream())
    if launch == "max_blocks_3":
        tree.tune(3)  # a workgroup walks ~90 chunks: the LDS partials are reused
    partials = torch.full((tree.n_chunks,), float("nan"), dtype=torch.float64, device=DEV)
    if launch == "buckets":
        for b in reversed(range(tree.n_buckets)):  # each writes exactly its chunk range
            K.grad_sumsq(tree, b, SLOT_GRAD, partials)
    else:
        K.grad_sumsq(tree, ALL, SLOT_GRAD, partials)
    assert partials.cpu().numpy().tobytes() == ref["parts"].tobytes()
    for max_norm in (float(ref["norm"]) / 2, float(ref["norm"]) * 2, 1.0):
        norm, coef = cr.finish(ref["parts"], max_norm)
        got = _finish(partials, max_norm).cpu().numpy()
        assert got[0].tobytes() == norm.tobytes() and got[1].tobytes() == coef.tobytes()
    assert _bits(grads) == _bits(torch.from_numpy(v) for v in ref["vals"])  # read only


def test_misaligned_bits_equal_aligned_bits(ref, tree):
    got = []
    for mis in (False, True):
        grads = _on_device(ref["vals"], mis)
        tree.bind(SLOT_GRAD, grads, _stream())
        partials = torch.zeros(tree.n_chunks, dtype=torch.float64, device=DEV)
        K.grad_sumsq(tree, ALL, SLOT_GRAD, partials)
        got.append((partials.cpu().numpy().tobytes(), _finish(partials, 1.0).cpu().numpy().tobytes()))
    assert got[0] == got[1]


def test_norm_against_torch_fp64_on_the_cpu(ref):
    """Relative error <= 2^-23: 2^-24 from the final fp32 rounding, < 64 * 2^-53 from the fp64
    tree (depth < 64), the sqrt halving the latter and adding one fp64 rounding."""
    ps = _params(ref["vals"])
    norm = utils.clip_grad_norm_(ps, float("inf"))
    want = float(torch.linalg.vector_norm(torch.cat(
        [torch.from_numpy(v).double() for v in ref["vals"]])))
    err = abs(float(norm) - want) / want
    print(f"norm {float(norm)!r} fp64 {want!r} relative error {err:.3e} bound {2.0 ** -23:.3e}")
    assert norm.dtype == torch.float32 and norm.dim() == 0 and norm.device == ps[0].device
    assert err <= 2.0 ** -23


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
def test_clipping_scales_by_torchs_coefficient(ref, misaligned):
    ps = _params(ref["vals"], misaligned)
    max_norm = float(ref["norm"]) / 2
    norm = utils.clip_grad_norm_(ps, max_norm)
    assert np.float32(norm.item()).tobytes() == ref["norm"].tobytes()
    # torch's own operations on the CPU, from the kernel's fp32 norm
    coef = torch.clamp(max_norm / (norm.cpu() + 1e-6), max=1.0)
    assert float(coef) < 1
    for p, v in zip(ps, ref["vals"]):
        assert torch.equal(p.grad.cpu(), torch.from_numpy(v) * coef)


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
def test_not_clipping_leaves_every_gradient_untouched(ref, misaligned):
    ps = _params(ref["vals"], misaligned)
    ptrs = [p.grad.data_ptr() for p in ps]
    norm = utils.clip_grad_norm_(ps, float(ref["norm"]) * 2)
    assert np.float32(norm.item()).tobytes() == ref["norm"].tobytes()
    assert [p.grad.data_ptr() for p in ps] == ptrs
    assert _bits(p.grad for p in ps) == _bits(torch.from_numpy(v) for v in ref["vals"])


@pytest.mark.parametrize("wire_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("divisor", [1, 2, 8])
@pytest.mark.parametrize("dst", ["slot", "slot_misaligned", "packed"])
def test_unpack_avg_sumsq_equals_unpack_avg_then_grad_sumsq(ref, tree, wire_dtype, divisor, dst):
    wire = torch.zeros(tree.total, dtype=torch.float32, device=DEV)
    src = _on_device(_values(12, scale=5.0))
    tree.bind(SLOT_AUX, src, _stream())
    K.gather(tree, ALL, SLOT_AUX, wire)
    wire = wire.to(wire_dtype)

    def run(fused):
        """(destination bytes, partials bytes) of the fused kernel or of the separate pair."""
        partials = torch.full((tree.n_chunks,), float("nan"), dtype=torch.float64, device=DEV)
        if dst == "packed":
            packed = torch.zeros(tree.total, dtype=torch.float32, device=DEV)
            outs = [packed[int(o):int(o) + n] for o, n in zip(tree.seg_off[:-1], NUMELS)]
            slot, dp = -1, packed
        else:
            outs = _on_device([np.zeros(n, np.float32) for n in NUMELS], dst == "slot_misaligned")
            slot, dp = SLOT_GRAD, None
        tree.bind(SLOT_GRAD, outs, _stream())
        if fused:
            for b in range(tree.n_buckets):
                K.unpack_avg_sumsq(tree, b, wire, divisor, slot, partials, dp)
        else:
            for b in range(tree.n_buckets):
                K.unpack_avg(tree, b, wire, divisor, slot, dp)
            K.grad_sumsq(tree, ALL, SLOT_GRAD, partials)
        return _bits(outs), partials.cpu().numpy().tobytes()

    fused, separate = run(True), run(False)
    assert fused[0] == separate[0], "destination bytes differ from dl_unpack_avg's"
    assert fused[1] == separate[1], "partials differ from dl_grad_sumsq on the destination"
    assert not np.isnan(np.frombuffer(fused[1], dtype=np.float64)).any()


@pytest.mark.parametrize("factor", [0.5, 2.0], ids=["clipping", "not_clipping"])
def test_gradsync_with_max_norm_equals_sync_then_clip_local(ref, factor):
    max_norm = float(ref["norm"]) * factor
    pa, pb = _params(ref["vals"]), _params(ref["vals"])
    ga = GradSync(pa, None, 1, bucket_cap_elems=CAP)
    gb = GradSync(pb, None, 1, bucket_cap_elems=CAP)
    assert ga.local and ga.tree.n_buckets >= 3
    na = ga.sync(max_norm)
    assert gb.sync() is None
    nb = utils.clip_grad_norm_(pb, max_norm)
    assert na.dtype == torch.float32 and na.dim() == 0
    assert np.float32(na.item()).tobytes() == np.float32(nb.item()).tobytes() == ref["norm"].tobytes()
    assert _bits(p.grad for p in pa) == _bits(p.grad for p in pb)
    changed = _bits(p.grad for p in pa) != _bits(torch.from_numpy(v) for v in ref["vals"])
    assert changed == (factor < 1)
    ga.close()
    gb.close()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker_rccl(rank, port, out):
    for p in (PKG, REPO, os.path.join(REPO, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from datetime import timedelta

    import torch.distributed as dist

    torch.cuda.set_device(0)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    dist.init_process_group("nccl", device_id=torch.device("cuda", 0),
                            timeout=timedelta(seconds=120))
    vals = _values()
    norm, _ = cr.norm_and_coef(vals, 1.0)
    rec = {"ref_norm": np.array([norm])}
    for exchange in ("rccl", "a2a"):
        for tag, factor in (("clip", 0.5), ("keep", 2.0)):
            max_norm = float(norm) * factor
            pa, pb = _params(vals), _params(vals)
            ga = GradSync(pa, None, 1, bucket_cap_elems=CAP, exchange=exchange)
            gb = GradSync(pb, None, 1, bucket_cap_elems=CAP, exchange=exchange)
            na = ga.sync(max_norm)
            gb.sync()
            nb = utils.clip_grad_norm_(pb, max_norm)
            torch.cuda.synchronize()
            key = f"{exchange}_{tag}"
            rec[key + "_through_rccl"] = np.array([not ga.local and ga.tree.n_buckets >= 3])
            rec[key + "_norms"] = np.array([na.item(), nb.item()], dtype=np.float32)
            rec[key + "_equal"] = np.array([_bits(p.grad for p in pa) == _bits(p.grad for p in pb)])
            rec[key + "_changed"] = np.array([
                _bits(p.grad for p in pa) != _bits(torch.from_numpy(v) for v in vals)])
            ga.close()
            gb.close()
    np.savez(os.path.join(out, "clip.npz"), **rec)
    dist.destroy_process_group()


def test_gradsync_with_max_norm_through_a_one_rank_rccl_group():
    """Both exchanges over a real one-rank RCCL communicator (an identity reduction): the fused
    sync equals sync() then utils.clip_grad_norm_, bit for bit in norm and gradients."""
    import torch.multiprocessing as mp

    out = tempfile.mkdtemp(prefix="dl_clip_rccl_")
    mp.spawn(_worker_rccl, args=(_free_port(), out), nprocs=1, join=True)
    rec = dict(np.load(os.path.join(out, "clip.npz")))
    for exchange in ("rccl", "a2a"):
        for tag in ("clip", "keep"):
            key = f"{exchange}_{tag}"
            assert rec[key + "_through_rccl"][0], key
            a, b = rec[key + "_norms"]
            assert a.tobytes() == b.tobytes() == rec["ref_norm"][0].tobytes(), key
            assert rec[key + "_equal"][0], key
            assert rec[key + "_changed"][0] == (tag == "clip"), key


def _pattern(ts):
    x = np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in ts])
    return np.isnan(x).tobytes() + np.isinf(x).tobytes()


@pytest.mark.parametrize("case", ["nan", "inf", "zeros"])
def test_special_values_follow_torchs_finiteness_pattern(case):
    vals = _values(13, [5, 4097, 9000])
    if case == "zeros":
        vals = [np.zeros_like(v) for v in vals]
    else:
        vals[1][4096] = np.nan if case == "nan" else np.inf
    pa, pb = _params(vals), _params(vals)
    na = utils.clip_grad_norm_(pa, 1.0)
    nb = torch.nn.utils.clip_grad_norm_(pb, 1.0)
    assert _pattern([na]) == _pattern([nb])
    assert _pattern(p.grad for p in pa) == _pattern(p.grad for p in pb)
    if case == "zeros":
        assert float(na) == 0.0 and _bits(p.grad for p in pa) == _bits(p.grad for p in pb)
        utils.clip_grad_norm_(pa, 1.0, error_if_nonfinite=True)  # finite: no error
    else:
        with pytest.raises(RuntimeError, match="non-finite"):
            utils.clip_grad_norm_(_params(vals), 1.0, error_if_nonfinite=True)


def test_1e25_has_a_finite_norm_here():
    """The one deliberate difference from torch: the fp64 sum does not overflow where torch's
    fp32 accumulation does (|g| >~ 1.8e19)."""
    vals = _values(14, [5, 4097, 9000])
    vals[2][17] = 1e25
    norm, coef, want = cr.clip(vals, 1.0)
    assert np.isfinite(norm) and 0 < coef < 1
    ps = _params(vals)
    got = utils.clip_grad_norm_(ps, 1.0, error_if_nonfinite=True)
    assert np.float32(got.item()).tobytes() == norm.tobytes()
    assert _bits(p.grad for p in ps) == _bits(torch.from_numpy(w) for w in want)


def test_ten_calls_with_freshly_allocated_grads():
    """More rebinds than the staging ring has slots, no host synchronisation in between: every
    call clips exactly the gradients bound just before it."""
    numels = [1, 3, 5000, 64, 4097, 0, 12345]
    ps = [torch.nn.Parameter(torch.zeros(n, device=DEV)) for n in numels]
    vals, kept, norms = [], [], []
    for k in range(10):
        v = _values(100 + k, numels, scale=1.0 + k)
        for p, g in zip(ps, _on_device(v)):
            p.grad = g
        norms.append(utils.clip_grad_norm_(ps, 300.0))  # rounds 0, 1 do not clip
        vals.append(v)
        kept.append([p.grad for p in ps])
    torch.cuda.synchronize()
    for k in range(10):
        norm, coef, want = cr.clip(vals[k], 300.0)
        assert np.float32(norms[k].item()).tobytes() == norm.tobytes(), k
        assert _bits(kept[k]) == _bits(torch.from_numpy(w) for w in want), k
