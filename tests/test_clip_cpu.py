"""Gradient-norm clipping without a GPU: the numpy restatement of the kernels' summation order
against an exact sum, and the orchestration above the kernels (GradSync.sync(max_norm), DPSync,
utils.clip_grad_norm_ and its tree cache) on the checker backend."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import clip_restatement as cr
from clip_oracle_kernels import NEW_METHODS, ClipOracleKernels, as_params
from diloco_amd import kernels, utils
from diloco_amd.comm import DPSync, dp_sync_gradients
from diloco_amd.gradsync import GradSync

NUMELS = [1, 3, 4, 63, 4095, 4096, 4097, 8197, 4096 * 3 + 7]
U64 = 2.0 ** -53


def _grads(seed=0, numels=NUMELS, scale=1.0):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(n) * scale).astype(np.float32) for n in numels]


@pytest.fixture
def oracle_backend():
    k = ClipOracleKernels()
    kernels.set_default_kernels(k)
    utils._clip_cache.clear()
    yield k
    kernels.set_default_kernels(None)
    utils._clip_cache.clear()


@pytest.mark.parametrize("numels", [NUMELS, [4096 * 300 + 5], [2]])
def test_restatement_agrees_with_an_exact_sum(numels):
    """Σ g²: every term is non-negative and passes through fewer than 64 fp64 additions (17 in
    the lane, 6 butterfly steps, 3 waves, then ceil(chunks / 256) + 9 in the finish), so the
    relative error is below (1 + u)^64 - 1 <= 64u / (1 - 64u), u = 2^-53. The norm: the sqrt halves that and rounds once
    in fp64, the narrowing to fp32 adds 2^-24: within 2^-23 of the exact norm."""
    g = _grads(1, numels, scale=3.0)
    # the fp64 square of an fp32 value is exact; fsum adds them without error
    exact = math.fsum(x for t in g for x in (t.astype(np.float64) ** 2).tolist())
    parts = cr.tree_partials(g)
    assert parts.size == sum(-(-n // 4096) for n in numels)
    # the finish's fp64 sum, before the sqrt: restated here from the same pieces
    rounds = -(-parts.size // 256)
    pad = np.zeros(rounds * 256)
    pad[:parts.size] = parts
    acc = np.zeros(256)
    for r in pad.reshape(-1, 256):
        acc = acc + r
    total = float(cr.block_sum(acc))
    assert rounds + 9 + 26 < 64
    assert abs(total - exact) <= 64 * U64 / (1 - 64 * U64) * exact  # >= (1 + u)^64 - 1
    norm, _ = cr.finish(parts, 1.0)
    assert norm == np.float32(np.sqrt(total))
    assert abs(float(norm) - math.sqrt(exact)) <= 2.0 ** -23 * math.sqrt(exact)


def test_restated_coefficient_is_torchs_fp32_sequence():
    """max_norm / (norm + 1e-6) with a Python float on the left is reciprocal-then-multiply in
    torch, then clamp(max=1): the restatement (and the kernel) follow it bit for bit."""
    rng = np.random.default_rng(5)
    norms = np.concatenate([np.exp(rng.uniform(-20, 20, 400)), [0.0, np.inf, np.nan, 1e-6, 1.0]])
    for nrm in norms.astype(np.float32):
        for max_norm in (1.0, 0.3, 7.25, float(nrm) / 2, float(nrm) * 2):
            sumsq = np.float64(nrm) ** 2 if np.isfinite(nrm) else np.float64(nrm)
            norm, coef = cr.finish(np.array([sumsq]), max_norm)
            t = torch.tensor(float(norm), dtype=torch.float32)
            ref = torch.clamp(max_norm / (t + 1e-6), max=1.0)
            assert np.float32(ref.item()).tobytes() == coef.tobytes() or (
                math.isnan(ref.item()) and math.isnan(float(coef))), (nrm, max_norm)


@pytest.mark.parametrize("factor", [0.5, 2.0])
@pytest.mark.parametrize("cap", [4096, 64 << 20])
def test_gradsync_with_max_norm_equals_sync_then_restated_clip(factor, cap):
    g = _grads(2)
    norm0, _ = cr.norm_and_coef(g, 1.0)
    max_norm = float(norm0) * factor
    k = ClipOracleKernels()
    pa, pb = as_params(g), as_params(g)
    ga = GradSync(pa, None, 1, bucket_cap_elems=cap, kernels=k)
    gb = GradSync(pb, None, 1, bucket_cap_elems=cap, kernels=k)
    assert cap > 4096 or ga.tree.n_buckets >= 3
    got = ga.sync(max_norm)
    assert gb.sync() is None
    norm, coef, want = cr.clip([p.grad.numpy() for p in pb], max_norm)
    assert (coef < 1) == (factor < 1)
    assert got.dtype == torch.float32 and got.dim() == 0
    assert np.float32(got.item()).tobytes() == norm.tobytes()
    for p, w in zip(pa, want):
        assert p.grad.numpy().tobytes() == w.tobytes()
    # launch order of the fused form: every unpack carries the sum, then one finish, one scaling
    names = [n for n, _ in k.calls]
    nb = ga.tree.n_buckets
    assert names[:nb] == ["unpack_avg_sumsq"] * nb
    assert k.calls[nb:nb + 2] == [("norm_finish", None), ("scale_by", -1)]


def test_max_norm_none_calls_none_of_the_new_kernels(oracle_backend):
    k = oracle_backend
    ps = as_params(_grads(3))
    before = [p.grad.clone() for p in ps]
    assert GradSync(ps, None, 1, bucket_cap_elems=4096).sync() is None
    model = torch.nn.Module()
    model.ps = torch.nn.ParameterList(ps)
    world = SimpleNamespace(stage2ranks={0: [0]}, stage=0, curr_stage_group=None)
    assert DPSync(world).sync_gradients(model) is None
    assert dp_sync_gradients(world, model) is None
    assert not [n for n, _ in k.calls if n in NEW_METHODS]
    assert "unpack_avg" in [n for n, _ in k.calls]
    assert all(torch.equal(a, p.grad) for a, p in zip(before, ps))


def test_dpsync_one_peer_syncs_then_clips(oracle_backend):
    g = _grads(4)
    ps = as_params(g)
    model = torch.nn.Module()
    model.ps = torch.nn.ParameterList(ps)
    world = SimpleNamespace(stage2ranks={0: [0]}, stage=0, curr_stage_group=None)
    norm, coef, want = cr.clip(g, 0.25)
    got = dp_sync_gradients(world, model, 0.25)
    assert np.float32(got.item()).tobytes() == norm.tobytes() and coef < 1
    for p, w in zip(ps, want):
        assert p.grad.numpy().tobytes() == w.tobytes()
    assert [n for n, _ in oracle_backend.calls] == ["grad_sumsq", "norm_finish", "scale_by"]


@pytest.mark.parametrize("kw", [dict(), dict(norm_type=1.0), dict(norm_type=float("inf")),
                                dict(foreach=False)])
def test_cpu_grads_take_torchs_call_unchanged(kw):
    g = _grads(6)
    pa, pb = as_params(g), as_params(g)
    pa.append(torch.nn.Parameter(torch.zeros(3)))  # no grad: skipped, as in torch
    pb.append(torch.nn.Parameter(torch.zeros(3)))
    a = utils.clip_grad_norm_(pa, 0.5, **kw)
    b = torch.nn.utils.clip_grad_norm_(pb, 0.5, **kw)
    assert torch.equal(a, b) and a.dtype == b.dtype and a.shape == b.shape
    assert all(torch.equal(x.grad, y.grad) for x, y in zip(pa[:-1], pb[:-1]))
    with pytest.raises(RuntimeError, match="non-finite"):
        pa[0].grad[0] = float("nan")
        utils.clip_grad_norm_(pa, 0.5, error_if_nonfinite=True)


def test_other_dtypes_and_layouts_take_torchs_call(oracle_backend):
    p = torch.nn.Parameter(torch.zeros(8, 8))
    p.grad = torch.arange(64.0).view(8, 8).t()  # not contiguous
    q = torch.nn.Parameter(torch.zeros(5, dtype=torch.float64))
    q.grad = torch.ones(5, dtype=torch.float64)
    for ps in ([p], [q]):
        want = torch.linalg.vector_norm(ps[0].grad.double().reshape(-1))
        got = utils.clip_grad_norm_(ps, 1e9)
        assert abs(float(got) - float(want)) <= 1e-5 * float(want)
    assert not oracle_backend.calls


def test_device_path_error_if_nonfinite_raises_before_scaling(oracle_backend):
    g = _grads(7)
    g[2][1] = np.inf
    ps = as_params(g)
    with pytest.raises(RuntimeError, match="non-finite"):
        utils.clip_grad_norm_(ps, 1.0, error_if_nonfinite=True)
    assert [n for n, _ in oracle_backend.calls] == ["grad_sumsq", "norm_finish"]
    assert all(p.grad.numpy().tobytes() == a.tobytes() for p, a in zip(ps, g))


def test_tree_cache_is_bounded_and_closes_evicted_trees(oracle_backend):
    k = oracle_backend
    n = utils.CLIP_CACHE_SIZE
    for i in range(n + 2):
        utils.clip_grad_norm_(as_params(_grads(8, [5 + i, 4097])), 1.0)
    assert len(k.trees) == n + 2 and len(utils._clip_cache) == n
    assert [t.closed for t in k.trees] == [True, True] + [False] * n
    # a hit reuses its tree and makes it the most recent
    utils.clip_grad_norm_(as_params(_grads(9, [5 + 2, 4097])), 1.0)
    assert len(k.trees) == n + 2
    utils.clip_grad_norm_(as_params(_grads(9, [99])), 1.0)
    assert [t.closed for t in k.trees] == [True, True, False, True] + [False] * (n - 1)
