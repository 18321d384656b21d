"""The fused inner AdamW step on the GPU: dl_adamw_step against the numpy restatement of its
contract (tests/adamw_restatement.py) on tests/test_adamw_gpu.py's ragged tree -- an empty
tensor, tails under 4, chunk edges, a multi-chunk tensor, and (bucket cap 4096) several buckets
-- its coefficient against dl_scale_by, its argument checks, optim.InnerAdamW through the
reference's loop (get_optimizer on the CPU, .to(device), clip, step, scheduler) against stock
AdamW on CPU clones, and its error against torch's own device step."""
import functools
import json
import os

import numpy as np
import pytest
import torch
from torch.optim.lr_scheduler import LambdaLR

import clip_restatement as cr
from adamw_restatement import F, adamw_elementwise, scalars
from diloco_amd import _lib, utils
from diloco_amd.kernels import HipKernels, adamw_scalars, set_default_kernels
from diloco_amd.optim import InnerAdamW
from diloco_amd.plan import SLOT_GRAD, SLOT_INNER, PackedTree
from stock_adamw import StockPair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HYPER = dict(lr=0.01, betas=(0.9, 0.95), weight_decay=0.1)
EPS = 1e-8
RAGGED = [1, 3, 5, 4097, 0, 64, 65, 12345, 8191, 4096 * 3 + 7, 2]
CAP = 4096
ALL = _lib.ALL_BUCKETS
K = HipKernels()
COEF = 0.37


def _sc(t):
    return adamw_scalars(HYPER["lr"], *HYPER["betas"], HYPER["weight_decay"], EPS, float(t))


def _ref_sc(t):
    return scalars(HYPER["lr"], HYPER["betas"], HYPER["weight_decay"], EPS, t)


def _grads(rng):
    """Over four decades, with exact zeros."""
    out = []
    for n in RAGGED:
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 0, n)).astype(F)
        g[::5] = 0
        out.append(g)
    return out


@functools.lru_cache(None)
def _inputs():
    """θ0 and three steps' gradients, shared (and left unchanged) by the tests below."""
    rng = np.random.default_rng(41)
    return [rng.standard_normal(n).astype(F) for n in RAGGED], [_grads(rng) for _ in range(3)]


def _scaled(g, k):
    if k is None:
        return g
    with np.errstate(all="ignore"):
        return (g * F(k)).astype(F)  # one rounded fp32 multiply


@functools.lru_cache(None)
def _expected(k):
    """[(θ, exp_avg, exp_avg_sq) after step s] from a zero state, by the restatement."""
    th, grads = _inputs()
    th = list(th)
    m = [np.zeros(n, F) for n in RAGGED]
    v = [np.zeros(n, F) for n in RAGGED]
    out = []
    for s in (1, 2, 3):
        for t in range(len(RAGGED)):
            th[t], m[t], v[t] = adamw_elementwise(th[t], m[t], v[t],
                                                  _scaled(grads[s - 1][t], k), _ref_sc(s))
        out.append((list(th), list(m), list(v)))
    return out


def _tensors(host, misaligned):
    """Per-tensor device storage: separate allocations, or slices of one buffer at odd element
    offsets (4-B aligned only: the kernel's element-wise path)."""
    if not misaligned:
        return [torch.from_numpy(h.copy()).to(DEV) for h in host]
    base = torch.empty(sum(h.size for h in host) + len(host), device=DEV)
    out, o = [], 1
    for h in host:
        out.append(base[o:o + h.size])
        out[-1].copy_(torch.from_numpy(h))
        o += h.size + 1
    return out


class _State:
    """A tree over `numels` with θ and g bound per tensor and zero exp_avg / exp_avg_sq arenas.
    Its padding checks use zero as the sentinel; tests/test_footprint_gpu.py pins the footprint."""

    def __init__(self, theta, th_mis=False, g_mis=False, numels=RAGGED, cap=CAP):
        self.numels = list(numels)
        self.tree = PackedTree(self.numels, cap)
        self.m = torch.zeros(self.tree.total, device=DEV)
        self.v = torch.zeros(self.tree.total, device=DEV)
        self.offs = [int(o) for o in self.tree.seg_off[:-1]]
        self.theta = _tensors(theta, th_mis)
        self.grad = _tensors([np.zeros(n, F) for n in self.numels], g_mis)
        s = torch.cuda.current_stream().cuda_stream
        self.tree.bind(SLOT_INNER, self.theta, s)
        self.tree.bind(SLOT_GRAD, self.grad, s)

    def set_grads(self, host):
        for t, h in zip(self.grad, host):
            t.copy_(torch.from_numpy(h))

    def step(self, s, coef=None, per_bucket=False):
        for b in (range(self.tree.n_buckets) if per_bucket else [ALL]):
            K.adamw_step(self.tree, b, SLOT_INNER, SLOT_GRAD, self.m, self.v, _sc(s), coef)

    def packed(self, buf):
        b = buf.cpu().numpy()
        return [b[o:o + n].copy() for o, n in zip(self.offs, self.numels)]

    def padding_is_zero(self):
        mask = torch.ones(self.tree.total, dtype=torch.bool, device=DEV)
        for o, n in zip(self.offs, self.numels):
            mask[o:o + n] = False
        return not bool(self.m[mask].any()) and not bool(self.v[mask].any())

    def host(self, tensors):
        return [t.cpu().numpy() for t in tensors]


def _eq(got, want, what):
    for t, (a, b) in enumerate(zip(got, want)):
        n = int((a.view(np.uint32) != b.view(np.uint32)).sum())
        assert a.tobytes() == b.tobytes(), (what, t, n)


@pytest.mark.parametrize("per_bucket", [True, False])
@pytest.mark.parametrize("coef", [None, COEF])
@pytest.mark.parametrize("g_mis", [False, True])
@pytest.mark.parametrize("th_mis", [False, True])
def test_adamw_step_matches_the_restatement(th_mis, g_mis, coef, per_bucket):
    """Three steps from a zero state, θ and g each 16-B aligned or at odd element offsets, with
    and without the coefficient, bucket by bucket or in one launch: θ, exp_avg and exp_avg_sq
    bit-equal to adamw_elementwise on g * k formed in fp32; g unchanged; the arenas' padding
    still zero."""
    theta0, grads = _inputs()
    st = _State(theta0, th_mis, g_mis)
    assert st.tree.n_buckets > 2
    k = None if coef is None else torch.tensor([coef], device=DEV)
    for s in (1, 2, 3):
        st.set_grads(grads[s - 1])
        st.step(s, k, per_bucket)
        torch.cuda.synchronize()
        th, m, v = _expected(coef)[s - 1]
        _eq(st.host(st.theta), th, ("theta", s))
        _eq(st.packed(st.m), m, ("exp_avg", s))
        _eq(st.packed(st.v), v, ("exp_avg_sq", s))
        _eq(st.host(st.grad), grads[s - 1], ("grad", s))
        assert st.padding_is_zero()
    st.tree.close()


@pytest.mark.parametrize("c", [0.37, 1.0, 0.0, float("nan")])
def test_coef_equals_scale_by_then_step(c):
    """adamw_step(coef=c) against dl_scale_by(c) followed by adamw_step(coef=None) on a twin,
    two steps: θ, exp_avg and exp_avg_sq the same bits (a NaN coefficient included), and only
    the twin's gradients scaled."""
    theta0, grads = _inputs()
    one, two = _State(theta0), _State(theta0)
    k = torch.tensor([c], device=DEV)
    for s in (1, 2):
        one.set_grads(grads[s - 1])
        two.set_grads(grads[s - 1])
        one.step(s, k)
        K.scale_by(two.tree, ALL, SLOT_GRAD, k)
        two.step(s)
        torch.cuda.synchronize()
        for a, b in zip(one.theta + [one.m, one.v], two.theta + [two.m, two.v]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), s
        _eq(one.host(one.grad), grads[s - 1], ("grad", s))
        if c != 1.0:
            assert any(not torch.equal(a.view(torch.int32), b.view(torch.int32))
                       for a, b in zip(one.grad, two.grad))
    if c != c:
        assert bool(torch.isnan(one.m[:1]).all())
    one.tree.close()
    two.tree.close()


def test_special_values_match_the_restatement():
    """Gradients that are exactly 0 on a zero state (den = eps), |g| = 1e-30 (g*g underflows to
    zero), 1e-20 (g*g denormal) and 1e-38 (g itself denormal), both signs, three steps: the
    kernel keeps denormals and its sqrt and divisions are correctly rounded."""
    pat = np.array([0.0, 1e-30, -1e-30, 1e-20, -1e-20, 1e-38, -1e-38, 1.0, 0.0, -3e-5], F)
    g = [np.resize(pat, n).astype(F) for n in RAGGED]
    th = list(_inputs()[0])
    m = [np.zeros(n, F) for n in RAGGED]
    v = [np.zeros(n, F) for n in RAGGED]
    st = _State(th)
    st.set_grads(g)
    for s in (1, 2, 3):
        st.step(s)
        torch.cuda.synchronize()
        for t in range(len(RAGGED)):
            th[t], m[t], v[t] = adamw_elementwise(th[t], m[t], v[t], g[t], _ref_sc(s))
        _eq(st.host(st.theta), th, ("theta", s))
        _eq(st.packed(st.m), m, ("exp_avg", s))
        _eq(st.packed(st.v), v, ("exp_avg_sq", s))
    big = max(range(len(RAGGED)), key=RAGGED.__getitem__)
    assert v[big][0] == 0 and v[big][1] == 0 and 0 < v[big][3] < np.finfo(F).tiny
    st.tree.close()


def test_adamw_step_argument_errors_are_raised():
    tree = PackedTree([10, 20])
    s = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(tree.total, device=DEV)
    a = buf.data_ptr()
    sc = _sc(1)
    theta = [torch.ones(10, device=DEV), torch.ones(20, device=DEV)]
    grad = [torch.ones(10, device=DEV), torch.ones(20, device=DEV)]

    def call(t, bucket, m, v, coef=None):
        _lib.call("dl_adamw_step", t, bucket, SLOT_INNER, SLOT_GRAD, m, v, coef, *sc, s)

    with pytest.raises(_lib.DilocoHipError, match="not bound"):
        call(tree.handle, -1, a, a)
    tree.bind(SLOT_INNER, theta, s)
    with pytest.raises(_lib.DilocoHipError, match="not bound"):  # the gradient slot
        call(tree.handle, -1, a, a)
    tree.bind(SLOT_GRAD, grad, s)
    for args, msg in [((None, -1, a, a), "null tree"),
                      ((tree.handle, 5, a, a), "bucket"),
                      ((tree.handle, -1, None, a), "exp_avg is null"),
                      ((tree.handle, -1, a, None), "exp_avg_sq is null"),
                      ((tree.handle, -1, a + 4, a), "aligned"),
                      ((tree.handle, -1, a, a + 8), "aligned"),
                      ((tree.handle, -1, a, a, a + 2), "aligned")]:
        with pytest.raises(_lib.DilocoHipError, match=msg):
            call(*args)
    torch.cuda.synchronize()
    assert not buf.any()  # nothing was launched
    assert all(bool((t == 1).all()) for t in theta + grad)
    tree.close()


# ---- the drop-in surface -------------------------------------------------------------------
class _Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


# the reference's inner optimizer (configs/optimizer/adamw.toml) under its warm-up schedule
INNER_CFG = _Cfg(type="AdamW", lr=6e-4, betas=(0.9, 0.95), weight_decay=0.1)
SHAPES = [(7, 9), (1,), (4097,), (0,), (65,), (3, 1367)]
WARMUP = 4


def _warmup(step):
    return step / WARMUP if step < WARMUP else 1.0


def _dropin(fold, monkeypatch):
    """Four steps of the reference's loop; returns per step the bits of θ, exp_avg, exp_avg_sq,
    the step counts and the norms, after checking each step against stock AdamW."""
    monkeypatch.setenv("DILOCO_INNER_ADAMW", "fused")
    rng = np.random.default_rng(43)
    vals = [rng.standard_normal(s).astype(F) for s in SHAPES]
    model = torch.nn.Module()
    model.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(v.copy()))
                                       for v in vals])
    opt = utils.get_optimizer(model, INNER_CFG)  # while the model is on the CPU
    assert type(opt) is InnerAdamW and opt._tree is None
    model = model.to(DEV)
    params = list(model.parameters())
    sched = LambdaLR(opt, _warmup)
    ref = StockPair(vals, _warmup, lr=INNER_CFG.lr, betas=INNER_CFG.betas,
                    weight_decay=INNER_CFG.weight_decay)
    launches = []

    def spy(*a, _f=K.adamw_step):
        launches.append(a[-1] is not None)  # was a coefficient handed in?
        return _f(*a)

    K.adamw_step = spy
    set_default_kernels(K)
    rec = []
    try:
        for s in (1, 2, 3, 4):
            g = [(rng.standard_normal(sh) * 10.0 ** rng.uniform(-4, 0, sh)).astype(F)
                 for sh in SHAPES]
            norm0, _ = cr.norm_and_coef([x.reshape(-1) for x in g], 1.0)
            max_norm = float(norm0) / 2 if s == 2 else float(norm0) * 2  # clips on step 2 only
            opt.zero_grad()
            for p, x in zip(params, g):
                p.grad = torch.from_numpy(x).to(DEV)  # a fresh tensor every step
            if fold:
                norm = opt.clip_grad_norm_(max_norm)
                for p, x in zip(params, g):  # the fold leaves .grad unscaled
                    assert p.grad.cpu().numpy().tobytes() == x.tobytes()
                coef = cr.norm_and_coef([x.reshape(-1) for x in g], max_norm)[1]
                seen = [torch.from_numpy(cr.scaled(x, coef)) for x in g]
            else:
                norm = utils.clip_grad_norm_(params, max_norm)
                seen = [p.grad.cpu() for p in params]  # as the clip left them
            assert any(a.numpy().tobytes() != x.tobytes() for a, x in zip(seen, g)) == (s == 2)
            opt.step()
            sched.step()
            torch.cuda.synchronize()
            ref.step(seen)
            ref.check(params, opt, f"{'fold' if fold else 'clip'} step {s}")
            assert launches == [fold] * s  # one dl_adamw_step per step
            assert float(norm) == float(norm0)
            rec.append([p.detach().cpu().numpy().tobytes() for p in params]
                       + [opt.state[p][k].cpu().numpy().tobytes() for p in params
                          for k in ("exp_avg", "exp_avg_sq")])
    finally:
        set_default_kernels(None)
        del K.adamw_step  # the spy was an instance attribute over the class's method
    assert opt._tree.n_chunks == 7 and opt._m.device.type == "cuda"
    return rec


def test_dropin_inner_adamw(monkeypatch):
    """get_optimizer under the knob while the module is on the CPU, .to(device), LambdaLR;
    four steps of fresh gradients -> utils.clip_grad_norm_ (clipping on step 2 only) -> step
    -> scheduler: θ, exp_avg, exp_avg_sq and step bit-equal to stock AdamW(foreach=False) on
    CPU clones fed the device gradients as the clip left them (tests/stock_adamw.py), one
    dl_adamw_step per step; the same loop with InnerAdamW.clip_grad_norm_ folded into the step
    gives the same bits with the gradients left unscaled."""
    plain = _dropin(False, monkeypatch)
    folded = _dropin(True, monkeypatch)
    assert plain == folded


# ---- against torch's own device step -------------------------------------------------------
def _adamw64(theta0, grads):
    """The contract's formula in numpy float64 on the fp32 inputs, from a zero state."""
    lr, (b1, b2), wd = HYPER["lr"], HYPER["betas"], HYPER["weight_decay"]
    th = np.concatenate(theta0).astype(np.float64)
    m, v = np.zeros_like(th), np.zeros_like(th)
    for t, gs in enumerate(grads, 1):
        g = np.concatenate(gs).astype(np.float64)
        th = th * (1 - lr * wd)
        m = m + (1 - b1) * (g - m)
        v = v * b2 + (1 - b2) * g * g
        den = np.sqrt(v) / (1 - b2 ** t) ** 0.5 + EPS
        th = th + (-(lr / (1 - b1 ** t)) * m) / den
    return th, m, v


def _err(x, x64):
    return float(np.linalg.norm(np.concatenate(x).astype(np.float64) - x64) / np.linalg.norm(x64))


def test_error_is_within_twice_torchs_device_step():
    """The same inputs, three steps, g' = fp32(g * 0.37): err(x) = |x - x64| / |x64| (2-norms
    over the tree) against the formula in float64, for θ, exp_avg and exp_avg_sq; the fused
    step's error is at most twice that of torch's own AdamW on the device. Both are the same
    short chain of correctly rounded fp32 operations, associated differently by torch's HIP
    foreach kernels, so their errors are the same size (on the CPU the contract's are 6.8e-8,
    4.2e-8 and 5.5e-8 and a re-associated form stays within 15 % of them); a wrong formula --
    no decay, no bias correction, an unscaled gradient -- is at least 2e-3."""
    theta0, grads = _inputs()
    scaled = [[_scaled(g, COEF) for g in gs] for gs in grads]
    x64 = _adamw64(theta0, scaled)
    st = _State(theta0)
    k = torch.tensor([COEF], device=DEV)
    stock_p = [torch.nn.Parameter(torch.from_numpy(t.copy()).to(DEV)) for t in theta0]
    stock = torch.optim.AdamW(stock_p, eps=EPS, **HYPER)
    for s in (1, 2, 3):
        st.set_grads(grads[s - 1])
        st.step(s, k)
        for p, g in zip(stock_p, scaled[s - 1]):
            p.grad = torch.from_numpy(g).to(DEV)
        stock.step()
    torch.cuda.synchronize()
    fused = (st.host(st.theta), st.packed(st.m), st.packed(st.v))
    torchs = ([p.detach().cpu().numpy() for p in stock_p],
              [stock.state[p]["exp_avg"].cpu().numpy() for p in stock_p],
              [stock.state[p]["exp_avg_sq"].cpu().numpy() for p in stock_p])
    rec = {}
    for name, a, b, ref in zip(("theta", "exp_avg", "exp_avg_sq"), fused, torchs, x64):
        rec[name] = {"err_fused": _err(a, ref), "err_torch_device": _err(b, ref)}
    print("inner_adamw_parity " + json.dumps(rec))
    out = os.environ.get("DILOCO_INNER_ADAMW_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            json.dump({"test": "tests/test_inner_adamw_gpu.py::"
                               "test_error_is_within_twice_torchs_device_step",
                       "tree": RAGGED, "steps": 3, "coef": COEF, "hyper": HYPER,
                       "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                       "err": "2-norm of (x - x64) over 2-norm of x64, x64 the formula in "
                              "numpy float64 on the same fp32 inputs",
                       "bound": "err_fused <= 2 * err_torch_device", "measured": rec},
                      f, indent=1)
            f.write("\n")
    for name, r in rec.items():
        assert r["err_fused"] <= 2 * r["err_torch_device"], (name, r)
    st.tree.close()
