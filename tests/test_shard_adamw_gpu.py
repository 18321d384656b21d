"""The flat-shard AdamW kernels on the GPU: dl_shard_adamw and dl_shard_reduce_adamw against
the numpy restatement of the AdamW contract (tests/adamw_restatement.py) and the C oracle's
rank-order average (oracle.sum_avg), their argument checks, and the reference's four calls
with DILOCO_OUTER_ADAMW=fused on the sharded and rank-order exchanges over two gloo processes
on the one GPU (RCCL refuses two ranks on one device; the kernels are the product's)."""
import os
import socket
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from adamw_restatement import AdamWState, F, adamw_elementwise, bf16_round, scalars
from conftest import PKG, REPO
from diloco_amd import _lib, synth
from diloco_amd.kernels import HipKernels, adamw_scalars, set_default_kernels
from diloco_amd.plan import PackedTree
from diloco_amd.trees import get_tree
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HYPER = dict(lr=0.01, betas=(0.9, 0.95), weight_decay=0.1)
EPS = 1e-8
PAD = 64          # sentinel elements past the end of every buffer a kernel writes
SENTINEL = -7.25
K = HipKernels()


def _sc(t):
    return adamw_scalars(HYPER["lr"], *HYPER["betas"], HYPER["weight_decay"], EPS, float(t))


def _ref_sc(t):
    return scalars(HYPER["lr"], HYPER["betas"], HYPER["weight_decay"], EPS, t)


def _padded(host):
    """A device buffer of host.size + PAD elements: the values, then sentinels."""
    t = torch.full((host.size + PAD,), SENTINEL, device=DEV)
    t[:host.size].copy_(torch.from_numpy(host))
    return t


def _body(t, n):
    return t[:n].cpu().numpy()


def _sentinels_ok(*bufs):
    return all(bool((b[-PAD:] == SENTINEL).all()) for b in bufs)


def _to_wire(host, dtype):
    return torch.from_numpy(host).to(DEV).to(dtype)


def _bits(a, b, what):
    assert a.tobytes() == b.tobytes(), (what, int((a.view(np.uint32) != b.view(np.uint32)).sum()))


# ---- dl_shard_adamw --------------------------------------------------------------------------
@pytest.mark.parametrize("wire", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("divisor", [1, 3])
@pytest.mark.parametrize("n", [1, 3, 4096, 4097, 3 * 4096 + 7])
def test_shard_adamw_matches_the_restatement_and_the_walker(n, divisor, wire):
    """Three steps from a zero state on a flat shard: θ, exp_avg and exp_avg_sq bit-equal to
    the restatement, the wire only read, the 64 elements past n of every written buffer
    untouched -- and the same inputs through dl_unpack_adamw on a one-tensor tree (the same
    body under the tree walker) give the same bits."""
    rng = np.random.default_rng(100 * n + divisor)
    th = rng.standard_normal(n).astype(F)
    m, v = np.zeros(n, F), np.zeros(n, F)
    d_th, d_m, d_v = _padded(th), _padded(m), _padded(v)
    tree = PackedTree([n], 4096)
    t_th = torch.zeros(tree.total, device=DEV)
    t_th[:n].copy_(torch.from_numpy(th))
    t_m, t_v = torch.zeros_like(t_th), torch.zeros_like(t_th)
    for s in (1, 2, 3):
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 0, n) * divisor).astype(F)
        g[::5] = 0
        if wire == torch.bfloat16:
            g = bf16_round(g)
        d_w = _to_wire(g, wire)
        t_w = torch.zeros(tree.total, dtype=wire, device=DEV)
        t_w[:n].copy_(d_w)
        K.shard_adamw(d_w, divisor, d_th[:n], d_m[:n], d_v[:n], _sc(s))
        K.unpack_adamw(tree, _lib.ALL_BUCKETS, t_w, divisor, t_th, t_m, t_v, _sc(s), -1)
        torch.cuda.synchronize()
        gg = g if divisor == 1 else g / F(divisor)
        th, m, v = adamw_elementwise(th, m, v, gg, _ref_sc(s))
        _bits(_body(d_th, n), th, ("theta", s))
        _bits(_body(d_m, n), m, ("exp_avg", s))
        _bits(_body(d_v, n), v, ("exp_avg_sq", s))
        _bits(d_w.float().cpu().numpy(), g, ("wire", s))
        assert _sentinels_ok(d_th, d_m, d_v), s
        for a, b in ((d_th, t_th), (d_m, t_m), (d_v, t_v)):
            assert torch.equal(a[:n], b[:n]), s
    tree.close()


# ---- dl_shard_reduce_adamw -------------------------------------------------------------------
LENS = [4, 2044, 2048, 2052, 4100, 3 * 4096 + 8]


def _slices(rng, n_slices, length, bf16):
    """n_slices x length values of mixed signs over four decades (fp32) or eight (bf16: its 8
    mantissa bits over four decades fit fp32's 24, and every order would give the same sum).
    Element 0 holds 1, 0, ..., 2^-24, 2^-24 at n_slices >= 3: in rank order 1 absorbs each
    2^-24 (a tie, to even), in any order that adds the two small terms first it does not."""
    span = 8 if bf16 else 4
    s = (rng.standard_normal((n_slices, length))
         * 10.0 ** rng.uniform(-span, 0, (n_slices, length))).astype(F)
    if n_slices >= 3:
        s[:, 0] = 0
        s[0, 0] = 1
        s[-2:, 0] = F(2.0 ** -24)
    return bf16_round(s.reshape(-1)).reshape(n_slices, length) if bf16 else s


def _sum_in_order(s, order):
    acc = s[order[0]].copy()
    for q in order[1:]:
        acc = acc + s[q]
    return acc


@pytest.mark.parametrize("with_avg", [True, False])
@pytest.mark.parametrize("wire", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n_slices", [1, 2, 3, 8, 9])
def test_shard_reduce_adamw_matches_rank_order_average_and_restatement(n_slices, wire, with_avg):
    """n_slices 1 (no division), 2 (four float4 rows per lane), 3 and 8 (two rows) and 9 (the
    run-time loop), at lengths on both sides of both row counts' workgroup edges (2048 and 4096
    elements) and more than one workgroup: two steps from a zero state; θ, exp_avg, exp_avg_sq
    and avg_out bit-equal to oracle.sum_avg + the restatement, the slices only read, the 64
    elements past `len` of every written buffer untouched. The inputs make the order of the sum
    visible: checked here on the CPU first, so a kernel summing in another order cannot pass."""
    bf16 = wire == torch.bfloat16
    for length in LENS:
        rng = np.random.default_rng(1000 * n_slices + length)
        th = rng.standard_normal(length).astype(F)
        m, v = np.zeros(length, F), np.zeros(length, F)
        d_th, d_m, d_v = _padded(th), _padded(m), _padded(v)
        d_avg = _padded(np.zeros(length, F)) if with_avg else None
        for s in (1, 2):
            sl = _slices(rng, n_slices, length, bf16)
            if n_slices >= 3:
                fwd = _sum_in_order(sl, list(range(n_slices)))
                rev = _sum_in_order(sl, list(range(n_slices))[::-1])
                assert (fwd != rev).any(), (n_slices, length)
            d_sl = _to_wire(sl.reshape(-1), wire)
            K.shard_reduce_adamw(d_sl, n_slices, d_th[:length], d_m[:length], d_v[:length],
                                 _sc(s), avg_out=None if d_avg is None else d_avg[:length])
            torch.cuda.synchronize()
            g = oracle.sum_avg([np.ascontiguousarray(x) for x in sl])
            th, m, v = adamw_elementwise(th, m, v, g, _ref_sc(s))
            what = (length, s)
            _bits(_body(d_th, length), th, ("theta",) + what)
            _bits(_body(d_m, length), m, ("exp_avg",) + what)
            _bits(_body(d_v, length), v, ("exp_avg_sq",) + what)
            _bits(d_sl.float().cpu().numpy(), sl.reshape(-1), ("slices",) + what)
            assert _sentinels_ok(d_th, d_m, d_v), what
            if with_avg:
                _bits(_body(d_avg, length), g, ("avg_out",) + what)
                assert _sentinels_ok(d_avg), what


# ---- special values --------------------------------------------------------------------------
def test_special_values_match_the_restatement():
    """Through both kernels, two steps: g = 0 on a zero state (den = eps), +-inf and NaN (θ, m
    and v become inf / NaN as IEEE arithmetic makes them), |g| = 1e-30 (g*g underflows to
    zero), 1e-20 (g*g, so v, denormal) and 1e-38 (g itself denormal). Bit for bit, NaNs
    included: each figure is printed before it is asserted."""
    pat = np.array([0.0, np.inf, -np.inf, np.nan, 1e-30, -1e-30, 1e-20, -1e-20, 1e-38, -1e-38,
                    1.0, 0.0, -3e-5], F)
    n = 4096 + 52  # a multiple of 4 past one chunk
    g = np.resize(pat, n).astype(F)
    rng = np.random.default_rng(5)
    theta0 = rng.standard_normal(n).astype(F)
    # the reduce kernel at one slice (g itself) and at two (g and zeros: (g + 0) / 2)
    cases = [("shard", None), ("reduce", 1), ("reduce", 2)]
    for kind, n_slices in cases:
        th, m, v = theta0.copy(), np.zeros(n, F), np.zeros(n, F)
        d_th, d_m, d_v = _padded(th), _padded(m), _padded(v)
        if kind == "shard":
            gg, d_g = g, torch.from_numpy(g).to(DEV)
        else:
            sl = np.concatenate([g] + [np.zeros(n, F)] * (n_slices - 1))
            gg = oracle.sum_avg([np.ascontiguousarray(sl[q * n:(q + 1) * n])
                                 for q in range(n_slices)])
            d_g = torch.from_numpy(sl).to(DEV)
        for s in (1, 2):
            if kind == "shard":
                K.shard_adamw(d_g, 1, d_th[:n], d_m[:n], d_v[:n], _sc(s))
            else:
                K.shard_reduce_adamw(d_g, n_slices, d_th[:n], d_m[:n], d_v[:n], _sc(s))
            torch.cuda.synchronize()
            th, m, v = adamw_elementwise(th, m, v, gg, _ref_sc(s))
            for name, got, want in (("theta", _body(d_th, n), th), ("exp_avg", _body(d_m, n), m),
                                    ("exp_avg_sq", _body(d_v, n), v)):
                diff = got.view(np.uint32) != want.view(np.uint32)
                print(f"{kind} n_slices={n_slices} step {s} {name}: {int(diff.sum())} differ, "
                      f"{int((diff & np.isnan(want)).sum())} of them NaN in the restatement")
            _bits(_body(d_th, n), th, (kind, n_slices, "theta", s))
            _bits(_body(d_m, n), m, (kind, n_slices, "exp_avg", s))
            _bits(_body(d_v, n), v, (kind, n_slices, "exp_avg_sq", s))
        assert v[4] == 0 and 0 < v[6] < np.finfo(F).tiny and np.isnan(th[1]) and np.isnan(m[3])


# ---- argument errors -------------------------------------------------------------------------
def test_argument_errors_are_raised_without_a_launch():
    n = 64
    bufs = [torch.full((n,), SENTINEL, device=DEV) for _ in range(5)]
    w, th, m, v, avg = (b.data_ptr() for b in bufs)
    s = torch.cuda.current_stream().cuda_stream
    sc = _sc(1)
    F32 = _lib.DL_F32
    for args, msg in [((w, F32, 2, 6, th, m, v, None), "multiple of 4"),
                      ((w, F32, 0, 8, th, m, v, None), "n_slices"),
                      ((w, F32, -1, 8, th, m, v, None), "n_slices"),
                      ((w, 7, 2, 8, th, m, v, None), "wire dtype"),
                      ((w, _lib.DL_F16, 2, 8, th, m, v, None), "wire dtype"),
                      ((w + 4, F32, 2, 8, th, m, v, None), "aligned"),
                      ((w, F32, 2, 8, th + 8, m, v, None), "aligned"),
                      ((w, F32, 2, 8, th, m + 4, v, None), "aligned"),
                      ((w, F32, 2, 8, th, m, v + 12, None), "aligned"),
                      ((w, F32, 2, 8, th, m, v, avg + 4), "aligned"),
                      ((None, F32, 2, 8, th, m, v, None), "slices is null"),
                      ((w, F32, 2, 8, None, m, v, None), "outer is null"),
                      ((w, F32, 2, 8, th, None, v, None), "exp_avg is null"),
                      ((w, F32, 2, 8, th, m, None, None), "exp_avg_sq is null")]:
        with pytest.raises(_lib.DilocoHipError, match=msg):
            _lib.call("dl_shard_reduce_adamw", *args, *sc, s)
    for args, msg in [((w, F32, 0, th, m, v, 8), "divisor"),
                      ((w, F32, 1, th, m, v, -4), "n -4"),
                      ((w, 7, 1, th, m, v, 8), "wire dtype"),
                      ((w + 4, F32, 1, th, m, v, 8), "aligned"),
                      ((w, F32, 1, th + 4, m, v, 8), "aligned"),
                      ((w, F32, 1, th, m + 8, v, 8), "aligned"),
                      ((w, F32, 1, th, m, v + 4, 8), "aligned"),
                      ((None, F32, 1, th, m, v, 8), "wire is null"),
                      ((w, F32, 1, None, m, v, 8), "outer is null"),
                      ((w, F32, 1, th, None, v, 8), "exp_avg is null"),
                      ((w, F32, 1, th, m, None, 8), "exp_avg_sq is null")]:
        with pytest.raises(_lib.DilocoHipError, match=msg):
            _lib.call("dl_shard_adamw", *args, *sc, s)
    with pytest.raises(TypeError, match="unsupported packed dtype"):
        K.shard_adamw(bufs[0].to(torch.float16), 1, bufs[1], bufs[2], bufs[3], sc)
    torch.cuda.synchronize()
    assert all(bool((b == SENTINEL).all()) for b in bufs)  # nothing was launched


# ---- the drop-in surface ---------------------------------------------------------------------
class _Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _flat(ts):
    return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in ts])


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


NEW = ("shard_adamw", "shard_reduce_adamw")
OLD = ("unpack_adamw", "delta_pack_adamw")


def _dropin(rank, world, exchange, device_placement, steps=3):
    """The reference's four calls with the fused AdamW outer optimizer on the micro tree in
    several buckets (this process = DP rank `rank` of `world`), beside the restatement on every
    rank's inner values. Every launch of the AdamW kernels is recorded by a counting wrapper
    installed with set_default_kernels, and every call of torch's own AdamW step body."""
    import diloco_amd.comm as comm_mod
    import torch.optim.adamw as torch_adamw
    from diloco_amd.comm import TrainingComm
    from diloco_amd.optim import OuterAdamW
    from diloco_amd.utils import (compute_pseudo_gradient, get_optimizer, get_outer_model,
                                  sync_inner_model)
    from diloco_amd.world import World

    comm_mod.DP_EXCHANGE = "a2a" if exchange == "a2a" else "rccl"
    spec = get_tree("micro")
    shapes = [s for _, s in spec.params()]
    theta0 = synth.outer_tree(spec.numels(), spec.init_spec())
    inner = torch.nn.Module()
    inner.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(v.copy()).view(s))
                                       for v, s in zip(theta0, shapes)])
    ref = AdamWState(theta0, **HYPER)
    launches, torch_steps = [], []
    for name in NEW + OLD:
        def spy(*a, _f=getattr(K, name), _n=name, **kw):
            launches.append(_n)
            return _f(*a, **kw)
        setattr(K, name, spy)
    stock_body = torch_adamw.adamw

    def counted_body(*a, **kw):
        torch_steps.append(1)
        return stock_body(*a, **kw)

    torch_adamw.adamw = counted_body
    set_default_kernels(K)
    rec = {}
    try:
        outer = get_outer_model(inner, "device" if device_placement else None,
                                exchange="sharded" if exchange == "sharded" else None)
        inner = inner.to(DEV)
        opt = get_optimizer(outer, _Cfg(type="AdamW", **HYPER))
        assert type(opt) is OuterAdamW
        comm = TrainingComm(World.from_default_group(1), (1, 1, 32), None)
        for s in range(1, steps + 1):
            vals = [synth.inner_tree(ref.theta, s, r) for r in range(world)]
            with torch.no_grad():
                for p, v in zip(inner.parameters(), vals[rank]):
                    p.copy_(torch.from_numpy(v).view(p.shape))
            n0 = len(launches)
            compute_pseudo_gradient(inner, outer)
            comm.sync_gradients(outer)
            opt.step()
            sync_inner_model(outer, inner)
            rec[f"launches_s{s}"] = np.array(launches[n0:])
            _, avg = ref.step(vals)
            torch.cuda.synchronize()
            rec[f"theta_s{s}"] = _flat(outer.parameters())
            rec[f"inner_s{s}"] = _flat(inner.parameters())
            rec[f"grad_s{s}"] = _flat(p.grad for p in outer.parameters())  # a collective read
            rec[f"ref_theta_s{s}"] = np.concatenate(ref.theta)
            rec[f"ref_grad_s{s}"] = np.concatenate(avg)
            if s >= 2:  # step 2 ran on the state step 1 left sharded; reading it gathers
                st = [opt.state[p] for p in outer.parameters()]
                rec[f"exp_avg_s{s}"] = _flat(x["exp_avg"] for x in st)
                rec[f"exp_avg_sq_s{s}"] = _flat(x["exp_avg_sq"] for x in st)
                rec[f"ref_exp_avg_s{s}"] = np.concatenate(ref.m)
                rec[f"ref_exp_avg_sq_s{s}"] = np.concatenate(ref.v)
                rec[f"step_s{s}"] = np.array([float(x["step"]) for x in st])
    finally:
        set_default_kernels(None)
        torch_adamw.adamw = stock_body
        for name in NEW + OLD:
            delattr(K, name)  # the spies were instance attributes over the class's methods
    m = outer._diloco_mirror
    rec["n_buckets"] = np.int64(getattr(m, "dev", m).tree.n_buckets)
    rec["torch_steps"] = np.int64(len(torch_steps))
    return rec


def _worker(rank, world, port, exchange, device_placement, out):
    for p in (PKG, REPO, os.path.join(REPO, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["DILOCO_DP_BACKEND"] = "gloo"
    os.environ["DILOCO_OUTER_ADAMW"] = "fused"
    os.environ["DILOCO_OUTER_BUCKET_ELEMS"] = "4096"
    os.environ.pop("DILOCO_OUTER_EXCHANGE", None)
    # a collective read its peer does not make fails fast instead of waiting
    os.environ["DILOCO_COLLECTIVE_READ_TIMEOUT"] = "10"
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank,
                            world_size=world)
    rec = _dropin(rank, world, exchange, device_placement)
    np.savez(os.path.join(out, f"r{rank}.npz"), **rec)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("placement", ["host", "device"])
@pytest.mark.parametrize("exchange", ["sharded", "a2a"])
def test_dropin_fused_adamw_two_peers_on_the_sharded_exchanges(exchange, placement):
    """Two gloo processes on the GPU, several buckets, three steps: after the reduce_scatter
    one dl_shard_adamw per bucket, after the all_to_all one dl_shard_reduce_adamw, then the
    all_gather of θ. (d0 + d1) / 2 has one order, so θ, inner, .grad, exp_avg and exp_avg_sq
    equal the restatement over the rank-order average bit for bit on both ranks, and the ranks
    agree. The new kernel ran n_buckets times per step; neither whole-tree AdamW kernel nor
    torch's own step body ran."""
    out = tempfile.mkdtemp(prefix="dl_shard_adamw_")
    mp.spawn(_worker, args=(2, _free_port(), exchange, placement == "device", out), nprocs=2,
             join=True)
    recs = [dict(np.load(os.path.join(out, f"r{r}.npz"))) for r in range(2)]
    kernel = "shard_adamw" if exchange == "sharded" else "shard_reduce_adamw"
    for rec in recs:
        nb = int(rec["n_buckets"])
        assert nb > 2
        assert int(rec["torch_steps"]) == 0
        for s in (1, 2, 3):
            assert list(rec[f"launches_s{s}"]) == [kernel] * nb, s
            assert rec[f"inner_s{s}"].tobytes() == rec[f"theta_s{s}"].tobytes(), s
            for key in ("theta", "grad"):
                got, want = rec[f"{key}_s{s}"], rec[f"ref_{key}_s{s}"]
                assert got.tobytes() == want.tobytes(), (key, s, int((got != want).sum()))
                assert got.tobytes() == recs[0][f"{key}_s{s}"].tobytes(), (key, s)
        for s in (2, 3):
            for key in ("exp_avg", "exp_avg_sq"):
                got, want = rec[f"{key}_s{s}"], rec[f"ref_{key}_s{s}"]
                assert got.tobytes() == want.tobytes(), (key, s, int((got != want).sum()))
                assert got.tobytes() == recs[0][f"{key}_s{s}"].tobytes(), (key, s)
            assert (rec[f"step_s{s}"] == s).all()
