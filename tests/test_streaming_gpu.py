"""The merging outer step on the GPU: dl_unpack_sgd_merge and dl_unpack_adamw_merge against the
numpy restatement of their contract (tests/streaming_restatement.py, tests/adamw_restatement.py)
on the ragged tree, bit for bit; their write footprint under non-zero sentinels; their argument
checks; and StreamingOuterSync on HipKernels against the simulator -- one replica, one replica
on a side stream behind a slow producer, and two gloo processes on the one GPU (RCCL refuses two
ranks on one device; the kernels are the product's)."""
import os
import socket
import sys
import tempfile
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import streaming_footprint as sfp
import streaming_restatement as sr
from adamw_restatement import F, adamw_elementwise, bf16_round, scalars
from conftest import PKG, REPO, spin
from diloco_amd import _lib, synth
from diloco_amd.kernels import HipKernels, adamw_scalars
from diloco_amd.plan import SLOT_AUX, SLOT_INNER, PackedTree
from diloco_amd.streaming import StreamingOuterSync
from diloco_amd.trees import get_tree
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# tests/test_kernels_gpu.py's ragged tree: an empty tensor, tails under 4, a 1-element chunk,
# chunk edges, and (bucket cap 4096) 7 buckets
RAGGED = [1, 3, 5, 4097, 0, 64, 65, 12345, 8191, 4096 * 3 + 7, 2]
CAP = 4096
ALL = _lib.ALL_BUCKETS
ALPHAS = (0.5, 0.3)
LR = 0.7
ADAM = dict(lr=0.01, betas=(0.9, 0.95), weight_decay=0.1)
EPS = 1e-8
K = HipKernels()
# (label, momentum, nesterov, first)
SGD_MODES = [("momentum0", 0.0, False, False), ("first", 0.9, True, True),
             ("nesterov", 0.9, True, False), ("plain", 0.9, False, False)]
HYPER = dict(lr=0.7, momentum=0.9, nesterov=True)
ENGINE_CASES = [(2, 1, 0, 0.0, "strided"), (4, 2, 1, 0.5, "strided"), (6, 3, 3, 0.3, "strided"),
                (6, 3, 3, 0.3, "sequential")]


def _sc(t):
    return adamw_scalars(ADAM["lr"], *ADAM["betas"], ADAM["weight_decay"], EPS, float(t))


def _ref_sc(t):
    return scalars(ADAM["lr"], ADAM["betas"], ADAM["weight_decay"], EPS, t)


def _inner_tensors(host, misaligned):
    """Per-tensor device storage: separate allocations, or slices of one buffer at odd element
    offsets (4-B aligned only: the kernels' element-wise path)."""
    if not misaligned:
        return [torch.from_numpy(h.copy()).to(DEV) for h in host]
    base = torch.empty(sum(RAGGED) + len(RAGGED), device=DEV)
    out, o = [], 1
    for h in host:
        out.append(base[o:o + h.size])
        out[-1].copy_(torch.from_numpy(h))
        o += h.size + 1
    return out


class _Packed:
    """θ, two state buffers and a wire in a PackedTree's layout, with per-tensor access. Its
    padding checks use zero as the sentinel; the footprint test below uses the non-zero ones."""

    def __init__(self, wire_dtype=torch.float32, max_blocks=0):
        self.tree = PackedTree(RAGGED, CAP)
        assert self.tree.n_buckets == 7
        if max_blocks:
            self.tree.tune(max_blocks)
        z = dict(dtype=torch.float32, device=DEV)
        self.theta = torch.zeros(self.tree.total, **z)
        self.m = torch.zeros(self.tree.total, **z)
        self.v = torch.zeros(self.tree.total, **z)
        self.wire = torch.zeros(self.tree.total, dtype=wire_dtype, device=DEV)
        self.offs = [int(o) for o in self.tree.seg_off[:-1]]

    def put(self, buf, host):
        for o, h in zip(self.offs, host):
            buf[o:o + h.size].copy_(torch.from_numpy(np.ascontiguousarray(h)).to(buf.dtype))

    def get(self, buf):
        b = buf.float().cpu().numpy()
        return [b[o:o + n].copy() for o, n in zip(self.offs, RAGGED)]

    def padding_is_zero(self, *bufs):
        mask = torch.ones(self.tree.total, dtype=torch.bool, device=DEV)
        for o, n in zip(self.offs, RAGGED):
            mask[o:o + n] = False
        return not any(bool(b[mask].any()) for b in bufs)

    def bind_inner(self, tensors):
        self.tree.bind(SLOT_INNER, tensors, torch.cuda.current_stream().cuda_stream)

    def buckets(self, launch):
        return [ALL] if launch == "whole" else list(range(self.tree.n_buckets))


def _eq(got, want, what):
    for t, (a, b) in enumerate(zip(got, want)):
        assert a.tobytes() == b.tobytes(), (what, t, int((a != b).sum()))


def _host(tensors):
    return [x.cpu().numpy() for x in tensors]


def _grads(rng, scale=1.0):
    """Over four decades, with exact zeros."""
    out = []
    for n in RAGGED:
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 0, n) * scale).astype(F)
        g[::5] = 0
        out.append(g)
    return out


def _inputs(seed, wire, divisor):
    rng = np.random.default_rng(seed)
    th = [rng.standard_normal(n).astype(F) for n in RAGGED]
    buf = [(rng.standard_normal(n) * 1e-2).astype(F) for n in RAGGED]
    g = _grads(rng, divisor)
    if wire == torch.bfloat16:
        g = [bf16_round(x) for x in g]
    # the inner model has moved on from θ by about the size of a step
    x = [(t + rng.standard_normal(t.size) * 1e-2).astype(F) for t in th]
    return th, buf, g, x


def _sgd_ref(th, buf, g, x, divisor, momentum, nesterov, first, alpha):
    th, buf = [t.copy() for t in th], [b.copy() for b in buf]
    inner = []
    for t, n in enumerate(RAGGED):
        gg = g[t] if divisor == 1 else (g[t] / F(divisor)).astype(F)
        if n:
            oracle.sgd(th[t], buf[t] if momentum else None, gg, LR, momentum, nesterov, first)
        inner.append(sr.merge(x[t], th[t], alpha))
    return th, buf, inner


def _run_sgd_merge(p, launch, divisor, momentum, nesterov, first, slot, alpha, merge=True):
    for b in p.buckets(launch):
        if merge:
            K.unpack_sgd_merge(p.tree, b, p.wire, divisor, p.theta, p.m if momentum else None, LR,
                               momentum, nesterov, first, slot, alpha)
        else:
            K.unpack_sgd(p.tree, b, p.wire, divisor, p.theta, p.m if momentum else None, LR,
                         momentum, nesterov, first, slot)
    torch.cuda.synchronize()


# ---- the kernels against the restatement ---------------------------------------------------------
@pytest.mark.parametrize("mode", SGD_MODES, ids=[m[0] for m in SGD_MODES])
@pytest.mark.parametrize("divisor", [1, 3])
@pytest.mark.parametrize("wire", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("misaligned", [False, True], ids=["separate", "misaligned"])
def test_unpack_sgd_merge_matches_the_restatement(misaligned, wire, divisor, mode):
    """θ, the momentum and inner bit-equal to oracle.sgd followed by the restated merge, for both
    alphas, whole-tree and bucket by bucket; the wire is only read; padding stays zero."""
    _label, momentum, nesterov, first = mode
    th, buf, g, x = _inputs(41, wire, divisor)
    for alpha in ALPHAS:
        want_th, want_buf, want_in = _sgd_ref(th, buf, g, x, divisor, momentum, nesterov, first,
                                              alpha)
        for launch in ("whole", "buckets"):
            p = _Packed(wire)
            p.put(p.theta, th)
            p.put(p.m, buf)
            p.put(p.wire, g)
            inner = _inner_tensors(x, misaligned)
            p.bind_inner(inner)
            _run_sgd_merge(p, launch, divisor, momentum, nesterov, first, SLOT_INNER, alpha)
            what = (alpha, launch)
            _eq(p.get(p.theta), want_th, ("theta",) + what)
            _eq(p.get(p.m), want_buf if momentum else buf, ("momentum",) + what)
            _eq(_host(inner), want_in, ("inner",) + what)
            _eq(p.get(p.wire), g, ("wire",) + what)
            assert p.padding_is_zero(p.theta, p.m, p.wire)
            p.tree.close()


@pytest.mark.parametrize("divisor", [1, 3])
@pytest.mark.parametrize("wire", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("misaligned", [False, True], ids=["separate", "misaligned"])
def test_unpack_adamw_merge_matches_the_restatement(misaligned, wire, divisor):
    """Three steps from a zero state (t = 1 is the first step, t = 3 a steady one): θ, exp_avg,
    exp_avg_sq and inner bit-equal to adamw_restatement followed by the restated merge."""
    for alpha in ALPHAS:
        for launch in ("whole", "buckets"):
            rng = np.random.default_rng(43)
            th = [rng.standard_normal(n).astype(F) for n in RAGGED]
            m = [np.zeros(n, F) for n in RAGGED]
            v = [np.zeros(n, F) for n in RAGGED]
            x = [(t + rng.standard_normal(t.size) * 1e-2).astype(F) for t in th]
            p = _Packed(wire)
            p.put(p.theta, th)
            inner = _inner_tensors(x, misaligned)
            p.bind_inner(inner)
            for s in (1, 2, 3):
                g = _grads(rng, divisor)
                if wire == torch.bfloat16:
                    g = [bf16_round(y) for y in g]
                p.put(p.wire, g)
                for b in p.buckets(launch):
                    K.unpack_adamw_merge(p.tree, b, p.wire, divisor, p.theta, p.m, p.v, _sc(s),
                                         SLOT_INNER, alpha)
                torch.cuda.synchronize()
                for t in range(len(RAGGED)):
                    gg = g[t] if divisor == 1 else g[t] / F(divisor)
                    th[t], m[t], v[t] = adamw_elementwise(th[t], m[t], v[t], gg, _ref_sc(s))
                    x[t] = sr.merge(x[t], th[t], alpha)
                what = (alpha, launch, s)
                _eq(p.get(p.theta), th, ("theta",) + what)
                _eq(p.get(p.m), m, ("exp_avg",) + what)
                _eq(p.get(p.v), v, ("exp_avg_sq",) + what)
                _eq(_host(inner), x, ("inner",) + what)
                _eq(p.get(p.wire), g, ("wire",) + what)
                assert p.padding_is_zero(p.theta, p.m, p.v, p.wire)
            p.tree.close()


@pytest.mark.parametrize("wire", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_theta_and_state_equal_the_pair_it_replaces(wire):
    """θ and the state byte-equal to dl_unpack_sgd / dl_unpack_adamw with inner_slot -1 on the
    same inputs, which leave inner alone for a lerp to follow."""
    th, buf, g, x = _inputs(47, wire, 3)
    for _label, momentum, nesterov, first in SGD_MODES:
        one, two = _Packed(wire), _Packed(wire)
        for p in (one, two):
            p.put(p.theta, th)
            p.put(p.m, buf)
            p.put(p.wire, g)
        in1, in2 = _inner_tensors(x, False), _inner_tensors(x, False)
        one.bind_inner(in1)
        two.bind_inner(in2)
        _run_sgd_merge(one, "whole", 3, momentum, nesterov, first, SLOT_INNER, 0.5)
        _run_sgd_merge(two, "whole", 3, momentum, nesterov, first, -1, None, merge=False)
        assert torch.equal(one.theta, two.theta) and torch.equal(one.m, two.m)
        _eq(_host(in2), x, "inner of the pair's first half")
        assert not all(a.tobytes() == b.tobytes() for a, b in zip(_host(in1), x))
        one.tree.close()
        two.tree.close()
    one, two = _Packed(wire), _Packed(wire)
    sq = [(b * b).astype(F) for b in buf]
    for p in (one, two):
        p.put(p.theta, th)
        p.put(p.m, buf)
        p.put(p.v, sq)
        p.put(p.wire, g)
    in1, in2 = _inner_tensors(x, False), _inner_tensors(x, False)
    one.bind_inner(in1)
    two.bind_inner(in2)
    K.unpack_adamw_merge(one.tree, ALL, one.wire, 3, one.theta, one.m, one.v, _sc(3), SLOT_INNER,
                         0.3)
    K.unpack_adamw(two.tree, ALL, two.wire, 3, two.theta, two.m, two.v, _sc(3), -1)
    torch.cuda.synchronize()
    for a, b in ((one.theta, two.theta), (one.m, two.m), (one.v, two.v)):
        assert torch.equal(a, b)
    one.tree.close()
    two.tree.close()


@pytest.mark.parametrize("rule", ["sgd", "adamw"])
def test_alpha_zero_is_the_plain_unpack(rule):
    """alpha = 0 launches the non-merging kernel: every output, inner included, byte-equal to
    dl_unpack_sgd / dl_unpack_adamw with the inner write, and an inner full of NaN (never
    loaded) is overwritten."""
    th, buf, g, x = _inputs(53, torch.float32, 3)
    nan = [np.full(n, np.nan, F) for n in RAGGED]
    sq = [(b * b).astype(F) for b in buf]
    one, two = _Packed(), _Packed()
    for p in (one, two):
        p.put(p.theta, th)
        p.put(p.m, buf)
        p.put(p.v, sq)
        p.put(p.wire, g)
    in1, in2 = _inner_tensors(nan, True), _inner_tensors(nan, True)
    one.bind_inner(in1)
    two.bind_inner(in2)
    if rule == "sgd":
        _run_sgd_merge(one, "buckets", 3, 0.9, True, False, SLOT_INNER, 0.0)
        _run_sgd_merge(two, "buckets", 3, 0.9, True, False, SLOT_INNER, None, merge=False)
    else:
        K.unpack_adamw_merge(one.tree, ALL, one.wire, 3, one.theta, one.m, one.v, _sc(2),
                             SLOT_INNER, 0.0)
        K.unpack_adamw(two.tree, ALL, two.wire, 3, two.theta, two.m, two.v, _sc(2), SLOT_INNER)
        torch.cuda.synchronize()
    for a, b in ((one.theta, two.theta), (one.m, two.m), (one.v, two.v), (one.wire, two.wire)):
        assert torch.equal(a, b)
    _eq(_host(in1), _host(in2), "inner")
    _eq(_host(in1), one.get(one.theta), "inner = theta")
    assert not any(np.isnan(a).any() for a in _host(in1))
    one.tree.close()
    two.tree.close()


@pytest.mark.parametrize("rule", ["sgd", "adamw"])
def test_results_do_not_depend_on_the_grid(rule):
    """dl_tree_tune(max_blocks = 1) and (max_blocks = 3) give the bytes of the default grid."""
    th, buf, g, x = _inputs(59, torch.float32, 3)
    sq = [(b * b).astype(F) for b in buf]
    res = []
    for max_blocks in (0, 1, 3):
        p = _Packed(max_blocks=max_blocks)
        p.put(p.theta, th)
        p.put(p.m, buf)
        p.put(p.v, sq)
        p.put(p.wire, g)
        inner = _inner_tensors(x, max_blocks == 1)  # and not on the alignment either
        p.bind_inner(inner)
        if rule == "sgd":
            _run_sgd_merge(p, "whole", 3, 0.9, True, False, SLOT_INNER, 0.3)
        else:
            K.unpack_adamw_merge(p.tree, ALL, p.wire, 3, p.theta, p.m, p.v, _sc(2), SLOT_INNER, 0.3)
            torch.cuda.synchronize()
        res.append([p.theta.cpu(), p.m.cpu(), p.v.cpu(), np.concatenate(_host(inner))])
        p.tree.close()
    for other in res[1:]:
        for a, b in zip(res[0][:3], other[:3]):
            assert torch.equal(a, b)
        assert res[0][3].tobytes() == other[3].tobytes()
    want = _sgd_ref(th, buf, g, x, 3, 0.9, True, False, 0.3)[2] if rule == "sgd" else None
    if want is not None:
        assert res[0][3].tobytes() == np.concatenate(want).tobytes()


def test_special_values_in_the_inner():
    """NaN, +-Inf, +-0, a denormal and FLT_MAX in the inner against a finite θ: IEEE rules, no
    special case. The NaN positions are the restatement's and every other value is byte-equal; θ
    and the momentum are untouched by them."""
    th, buf, g, x = _inputs(61, torch.float32, 1)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-42, -1e-42,
                        np.finfo(F).max, -np.finfo(F).max], F)
    for t, n in enumerate(RAGGED):  # in the float4 rows, the tails and the short tensors
        for j in range(n):
            if j % 7 == 0 or j >= n - 3:
                x[t][j] = special[(j + t) % special.size]
    for misaligned in (False, True):
        for alpha in ALPHAS:
            want_th, want_buf, want_in = _sgd_ref(th, buf, g, x, 1, 0.9, True, False, alpha)
            p = _Packed()
            p.put(p.theta, th)
            p.put(p.m, buf)
            p.put(p.wire, g)
            inner = _inner_tensors(x, misaligned)
            p.bind_inner(inner)
            _run_sgd_merge(p, "whole", 1, 0.9, True, False, SLOT_INNER, alpha)
            _eq(p.get(p.theta), want_th, "theta")
            _eq(p.get(p.m), want_buf, "momentum")
            seen = 0
            for got, want in zip(_host(inner), want_in):
                nan = np.isnan(want)
                seen += int(nan.sum())
                assert (np.isnan(got) == nan).all()
                assert got[~nan].tobytes() == want[~nan].tobytes()
            assert seen > 0
            p.tree.close()


# ---- footprint -----------------------------------------------------------------------------------
@pytest.mark.parametrize("row", list(sfp.TREE_ROWS))
@pytest.mark.parametrize("wire", ["f32", "bf16"])
def test_merge_footprint(wire, row):
    """Both sentinels, inner at 0, 1 and mixed 0-3 elements off a 16-B boundary, whole-tree and
    bucket by bucket, grid caps 0, 1, 2 and 5: after every launch every byte of every buffer --
    θ, the state, the wire (only read), inner, all padding, the guards around every inner tensor
    and the other buckets -- equals the CPU reference's."""
    for case in sfp.TREE_ROWS[row](wire):
        sfp.run_case(case, K, DEV, grids=sfp.fpt.GRIDS)


# ---- argument checks -----------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["sgd", "adamw"])
def test_argument_checks(rule):
    th, buf, g, x = _inputs(67, torch.float32, 1)
    p = _Packed()
    p.put(p.theta, th)
    p.put(p.m, buf)
    p.put(p.wire, g)
    inner = _inner_tensors(x, False)
    p.bind_inner(inner)
    torch.cuda.synchronize()
    before = [p.theta.clone(), p.m.clone(), p.v.clone(), p.wire.clone()] + [t.clone() for t in inner]

    def call(slot, alpha):
        if rule == "sgd":
            K.unpack_sgd_merge(p.tree, ALL, p.wire, 1, p.theta, p.m, LR, 0.9, True, False, slot,
                               alpha)
        else:
            K.unpack_adamw_merge(p.tree, ALL, p.wire, 1, p.theta, p.m, p.v, _sc(1), slot, alpha)

    for slot, alpha, word in [(SLOT_INNER, -0.1, "alpha"), (SLOT_INNER, 1.0, "alpha"),
                              (SLOT_INNER, float("nan"), "alpha"),
                              (SLOT_INNER, float("inf"), "alpha"), (-1, 0.5, "inner_slot"),
                              (SLOT_AUX, 0.5, "inner_slot"), (-1, 0.0, "inner_slot")]:
        with pytest.raises(_lib.DilocoHipError, match=word) as e:
            call(slot, alpha)
        assert e.value.code == -1  # DL_E_ARG
    torch.cuda.synchronize()
    after = [p.theta, p.m, p.v, p.wire] + inner
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    p.tree.close()


# ---- the engine on HipKernels ------------------------------------------------------------------------
def _ragged_theta0():
    rng = np.random.default_rng(71)
    return [rng.standard_normal(n).astype(F) for n in RAGGED]


def _inner_step(params, rank, t):
    """The stand-in inner step on device tensors, on the current stream."""
    for i, p in enumerate(params):
        if p.numel():
            p.add_(torch.from_numpy(sr.perturbation(rank, t, i, p.numel())).to(p.device))


def _flat(ts):
    return np.concatenate([t.detach().float().cpu().numpy().reshape(-1) for t in ts])


def _state(eng, params, wire=True):
    out = {"theta": _flat(eng.unpacked(eng.theta)), "mom": _flat(eng.unpacked(eng.mom)),
           "inner": _flat(params)}
    if wire:
        out["wire"] = _flat(eng.unpacked(eng.wire))
    return out


def _same(got, sim, what, rank=0):
    for k, v in got.items():
        w = sim.flat(k, rank)
        assert v.tobytes() == w.tobytes(), (what, k, int((v != w).sum()))


@pytest.mark.parametrize("H,P,tau,alpha,pattern", ENGINE_CASES)
def test_engine_one_replica_matches_the_simulator(H, P, tau, alpha, pattern):
    theta0 = _ragged_theta0()
    params = [torch.from_numpy(t.copy()).to(DEV) for t in theta0]
    eng = StreamingOuterSync(params, sync_every=H, fragments=P, delay=tau, alpha=alpha,
                             pattern=pattern, bucket_cap_elems=CAP, world_size=1, kernels=K,
                             **HYPER)
    sim = sr.StreamSim(theta0, 1, H, P, tau, alpha, CAP, pattern, **HYPER)
    assert eng.tree.n_buckets == 7 and eng.fragment_buckets == sim.frags and eng.stream is None
    for t in range(1, 2 * H + 2):
        _inner_step(params, 0, t)
        sim.inner_steps()
        eng.after_inner_step()
        sim.after_inner_step()
        assert eng.in_flight == list(sim.open) and eng.bucket_steps == sim.bucket_steps
        _same(_state(eng, params), sim, (H, P, tau, t))
    eng.flush()
    sim.flush()
    _same(_state(eng, params), sim, "flush")
    eng.close()


def test_engine_reads_the_inner_values_stream_order_gives_it():
    """Everything on a side stream, every inner stand-in queued behind a 50 ms dl_spin on that
    stream (a slow producer, as in tests/test_async_order_gpu.py): begin and finish read the inner
    values that stream order gives them, so the run equals the simulator; an engine that launched
    on another stream would read the values of the step before."""
    H, P, tau, alpha = 4, 2, 1, 0.5
    theta0 = _ragged_theta0()
    params = [torch.from_numpy(t.copy()).to(DEV) for t in theta0]
    sim = sr.StreamSim(theta0, 1, H, P, tau, alpha, CAP, **HYPER)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        eng = StreamingOuterSync(params, sync_every=H, fragments=P, delay=tau, alpha=alpha,
                                 bucket_cap_elems=CAP, world_size=1, kernels=K, **HYPER)
        for t in range(1, 2 * H + 2):
            pert = [torch.from_numpy(sr.perturbation(0, t, i, p.numel())).to(DEV)
                    for i, p in enumerate(params)]
            side.synchronize()  # the perturbations are staged; nothing below waits on the host
            spin(50)
            for p, d in zip(params, pert):
                if p.numel():
                    p.add_(d)
            eng.after_inner_step()
            busy = not side.query()  # the launches were queued while the producer still ran
            sim.inner_steps()
            sim.after_inner_step()
            side.synchronize()
            assert busy
            _same(_state(eng, params), sim, t)
        eng.flush()
        sim.flush()
        side.synchronize()
        _same(_state(eng, params), sim, "flush")
    eng.close()


# ---- two gloo processes on the one GPU ---------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, case, steps, out):
    for p in (PKG, REPO, os.path.join(REPO, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank,
                            world_size=world)
    H, P, tau, alpha = case
    spec = get_tree("micro")
    theta0 = synth.outer_tree(spec.numels(), spec.init_spec())
    params = [torch.from_numpy(t.copy()).to(DEV) for t in theta0]
    eng = StreamingOuterSync(params, sync_every=H, fragments=P, delay=tau, alpha=alpha,
                             bucket_cap_elems=CAP, world_size=world, rank=rank,
                             kernels=HipKernels(), **HYPER)
    assert eng.tree.n_buckets == 12 and not eng._local()
    rec = {}
    for t in range(1, steps + 1):
        _inner_step(params, rank, t)
        eng.after_inner_step()
        for k, v in _state(eng, params, wire=False).items():
            rec[f"{k}_t{t}"] = v
    eng.flush()
    for k, v in _state(eng, params).items():
        rec[f"{k}_end"] = v
    np.savez(os.path.join(out, f"r{rank}.npz"), **rec)
    dist.barrier()
    dist.destroy_process_group()
    eng.close()


def test_two_gloo_ranks_on_the_gpu_match_the_simulator():
    """micro tree, 12 buckets, (H, P, tau, alpha) = (4, 2, 1, 0.5), 9 inner steps then flush():
    θ, the momentum and each rank's inner parameters after every call, and the wire at the end,
    bit-exact against the simulator on both ranks."""
    case, steps, world = (4, 2, 1, 0.5), 9, 2
    out = tempfile.mkdtemp(prefix="dl_stream_gpu_")
    ctx = mp.start_processes(_worker, args=(world, _free_port(), case, steps, out), nprocs=world,
                             join=False, start_method="spawn")  # a fresh child per rank
    deadline = time.time() + 120
    while not ctx.join(timeout=5):  # raises when a rank failed, and ends the other
        if time.time() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the two ranks did not finish within 120 s")
    spec = get_tree("micro")
    sim = sr.StreamSim(synth.outer_tree(spec.numels(), spec.init_spec()), world, *case, CAP,
                       **HYPER)
    recs = [dict(np.load(os.path.join(out, f"r{r}.npz"))) for r in range(world)]
    for t in range(1, steps + 1):
        sim.inner_steps()
        sim.after_inner_step()
        for r, rec in enumerate(recs):
            for k in ("theta", "mom", "inner"):
                assert rec[f"{k}_t{t}"].tobytes() == sim.flat(k, r).tobytes(), (r, k, t)
    sim.flush()
    for r, rec in enumerate(recs):
        for k in ("theta", "mom", "inner", "wire"):
            assert rec[f"{k}_end"].tobytes() == sim.flat(k, r).tobytes(), (r, k, "end")
