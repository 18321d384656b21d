"""The fused AdamW outer step on the GPU: dl_unpack_adamw and dl_delta_pack_adamw against the
numpy restatement of their contract (tests/adamw_restatement.py) on a ragged tree (and, beside
it, dl_unpack_sgd -- the same walker body with the SGD rule -- against the CPU oracle), and the
reference's four calls with DILOCO_OUTER_ADAMW=fused at one peer and over two gloo processes
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
from diloco_amd.plan import SLOT_INNER, PackedTree
from diloco_amd.trees import get_tree
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HYPER = dict(lr=0.01, betas=(0.9, 0.95), weight_decay=0.1)
EPS = 1e-8
# tests/test_kernels_gpu.py's ragged tree: an empty tensor, tails under 4, chunk edges, and
# (bucket cap 4096) several buckets
RAGGED = [1, 3, 5, 4097, 0, 64, 65, 12345, 8191, 4096 * 3 + 7, 2]
CAP = 4096
K = HipKernels()


def _sc(t):
    return adamw_scalars(HYPER["lr"], *HYPER["betas"], HYPER["weight_decay"], EPS, float(t))


def _ref_sc(t):
    return scalars(HYPER["lr"], HYPER["betas"], HYPER["weight_decay"], EPS, t)


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
    """θ, exp_avg, exp_avg_sq and a wire in a PackedTree's layout, with per-tensor access.
    Its padding checks use zero as the sentinel; tests/test_footprint_gpu.py pins the footprint."""

    def __init__(self, wire_dtype):
        self.tree = PackedTree(RAGGED, CAP)
        assert self.tree.n_buckets > 2
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


def _eq(got, want, what):
    for t, (a, b) in enumerate(zip(got, want)):
        assert a.tobytes() == b.tobytes(), (what, t, int((a != b).sum()))


def _grads(rng, scale=1.0):
    """Over four decades, with exact zeros."""
    out = []
    for n in RAGGED:
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 0, n) * scale).astype(F)
        g[::5] = 0
        out.append(g)
    return out


@pytest.mark.parametrize("bound", [True, False])
@pytest.mark.parametrize("divisor", [1, 3])
@pytest.mark.parametrize("wire", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("misaligned", [False, True])
def test_unpack_adamw_matches_the_restatement(misaligned, wire, divisor, bound):
    """dl_unpack_adamw bucket by bucket on the ragged tree, three steps from a zero state: θ,
    exp_avg, exp_avg_sq and the inner tensors (inner_slot -1: untouched) bit-equal to the
    restatement; the wire is only read; padding stays zero."""
    rng = np.random.default_rng(17)
    th = [rng.standard_normal(n).astype(F) for n in RAGGED]
    m = [np.zeros(n, F) for n in RAGGED]
    v = [np.zeros(n, F) for n in RAGGED]
    p = _Packed(wire)
    p.put(p.theta, th)
    inner0 = [rng.standard_normal(n).astype(F) for n in RAGGED]
    inner = _inner_tensors(inner0, misaligned)
    p.bind_inner(inner)
    for s in (1, 2, 3):
        g = _grads(rng, divisor)
        if wire == torch.bfloat16:
            g = [bf16_round(x) for x in g]
        p.put(p.wire, g)
        for b in range(p.tree.n_buckets):
            K.unpack_adamw(p.tree, b, p.wire, divisor, p.theta, p.m, p.v, _sc(s),
                           SLOT_INNER if bound else -1)
        torch.cuda.synchronize()
        for t in range(len(RAGGED)):
            gg = g[t] if divisor == 1 else g[t] / F(divisor)
            th[t], m[t], v[t] = adamw_elementwise(th[t], m[t], v[t], gg, _ref_sc(s))
        _eq(p.get(p.theta), th, ("theta", s))
        _eq(p.get(p.m), m, ("exp_avg", s))
        _eq(p.get(p.v), v, ("exp_avg_sq", s))
        _eq(p.get(p.wire), g, ("wire", s))
        _eq([x.cpu().numpy() for x in inner], th if bound else inner0, ("inner", s))
        assert p.padding_is_zero(p.theta, p.m, p.v, p.wire)
    p.tree.close()


@pytest.mark.parametrize("momentum,nesterov", [(0.9, True), (0.9, False), (0.0, False)])
@pytest.mark.parametrize("divisor", [1, 3])
@pytest.mark.parametrize("wire", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("inner", ["aligned", "misaligned", "unbound"])
def test_unpack_sgd_matches_the_oracle(inner, wire, divisor, momentum, nesterov):
    """The SGD twin: dl_unpack_sgd called directly, bucket by bucket on the ragged tree, one
    first and one steady step: θ, the momentum buffer and the inner tensors (inner_slot -1:
    untouched) byte-equal to the CPU oracle's division and SGD; the wire is only read; padding
    stays zero. Without a momentum the buffer is not passed and stays as it was."""
    rng = np.random.default_rng(29)
    th = [rng.standard_normal(n).astype(F) for n in RAGGED]
    buf = [np.zeros(n, F) for n in RAGGED]
    p = _Packed(wire)
    p.put(p.theta, th)
    inner0 = [rng.standard_normal(n).astype(F) for n in RAGGED]
    tensors = _inner_tensors(inner0, inner == "misaligned")
    p.bind_inner(tensors)
    slot = -1 if inner == "unbound" else SLOT_INNER
    stream = torch.cuda.current_stream().cuda_stream
    for first in (True, False):
        g = _grads(rng, divisor)
        if wire == torch.bfloat16:
            g = [bf16_round(x) for x in g]
        p.put(p.wire, g)
        for b in range(p.tree.n_buckets):
            _lib.call("dl_unpack_sgd", p.tree.handle, b, p.wire.data_ptr(),
                      _lib.DL_BF16 if wire == torch.bfloat16 else _lib.DL_F32, divisor,
                      p.theta.data_ptr(), p.m.data_ptr() if momentum else None, 0.7, momentum,
                      int(nesterov), int(first), slot, stream)
        torch.cuda.synchronize()
        for t, n in enumerate(RAGGED):
            gg = g[t] if divisor == 1 else (g[t] / F(divisor)).astype(F)
            if n:
                oracle.sgd(th[t], buf[t] if momentum else None, gg, 0.7, momentum, nesterov, first)
        _eq(p.get(p.theta), th, ("theta", first))
        _eq(p.get(p.m), buf, ("momentum", first))
        _eq(p.get(p.wire), g, ("wire", first))
        _eq([x.cpu().numpy() for x in tensors], inner0 if inner == "unbound" else th,
            ("inner", first))
        assert p.padding_is_zero(p.theta, p.m, p.wire)
    p.tree.close()


@pytest.mark.parametrize("wire", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("misaligned", [False, True])
def test_delta_pack_adamw_matches_the_restatement_and_the_pair(misaligned, wire):
    """dl_delta_pack_adamw over the whole ragged tree, three steps from a zero state: the wire
    (bf16: RNE, AdamW steps on the rounded value), θ, exp_avg, exp_avg_sq and inner bit-equal
    to the restatement -- and to dl_delta_pack followed by dl_unpack_adamw with divisor 1, run
    beside it on copies, wire included."""
    rng = np.random.default_rng(23)
    theta0 = [rng.standard_normal(n).astype(F) for n in RAGGED]
    st = AdamWState(theta0, eps=EPS, **HYPER)
    one, two = _Packed(wire), _Packed(wire)
    one.put(one.theta, theta0)
    two.put(two.theta, theta0)
    in1 = _inner_tensors(theta0, misaligned)
    in2 = _inner_tensors(theta0, misaligned)
    one.bind_inner(in1)
    two.bind_inner(in2)
    for s in (1, 2, 3):
        vals = [(t + z).astype(F) for t, z in zip(st.theta, _grads(rng, 1e-2))]
        for a, b, x in zip(in1, in2, vals):
            a.copy_(torch.from_numpy(x))
            b.copy_(torch.from_numpy(x))
        K.delta_pack_adamw(one.tree, _lib.ALL_BUCKETS, SLOT_INNER, one.theta, one.wire, one.m,
                           one.v, _sc(s))
        for b in range(two.tree.n_buckets):
            K.delta_pack(two.tree, b, SLOT_INNER, two.theta, two.wire)
        for b in range(two.tree.n_buckets):
            K.unpack_adamw(two.tree, b, two.wire, 1, two.theta, two.m, two.v, _sc(s), SLOT_INNER)
        torch.cuda.synchronize()
        deltas, _ = st.step([vals], wire="bf16" if wire == torch.bfloat16 else "f32")
        for p, inner in ((one, in1), (two, in2)):
            _eq(p.get(p.wire), deltas[0], ("wire", s))
            _eq(p.get(p.theta), st.theta, ("theta", s))
            _eq(p.get(p.m), st.m, ("exp_avg", s))
            _eq(p.get(p.v), st.v, ("exp_avg_sq", s))
            _eq([x.cpu().numpy() for x in inner], st.theta, ("inner", s))
            assert p.padding_is_zero(p.theta, p.m, p.v, p.wire)
        for a, b in ((one.wire, two.wire), (one.theta, two.theta), (one.m, two.m), (one.v, two.v)):
            assert torch.equal(a, b)
    one.tree.close()
    two.tree.close()


def test_special_values_match_the_restatement():
    """Gradients that are exactly 0 on a zero state (den = eps), |g| = 1e-30 (g*g underflows to
    zero), 1e-20 (g*g denormal) and 1e-38 (g itself denormal), both signs, three steps: the
    kernel keeps denormals and its sqrt and divisions are correctly rounded."""
    pat = np.array([0.0, 1e-30, -1e-30, 1e-20, -1e-20, 1e-38, -1e-38, 1.0, 0.0, -3e-5], F)
    g = [np.resize(pat, n).astype(F) for n in RAGGED]
    rng = np.random.default_rng(5)
    th = [rng.standard_normal(n).astype(F) for n in RAGGED]
    m = [np.zeros(n, F) for n in RAGGED]
    v = [np.zeros(n, F) for n in RAGGED]
    p = _Packed(torch.float32)
    p.put(p.theta, th)
    p.put(p.wire, g)
    for s in (1, 2, 3):
        K.unpack_adamw(p.tree, _lib.ALL_BUCKETS, p.wire, 1, p.theta, p.m, p.v, _sc(s), -1)
        torch.cuda.synchronize()
        for t in range(len(RAGGED)):
            th[t], m[t], v[t] = adamw_elementwise(th[t], m[t], v[t], g[t], _ref_sc(s))
        _eq(p.get(p.theta), th, ("theta", s))
        _eq(p.get(p.m), m, ("exp_avg", s))
        _eq(p.get(p.v), v, ("exp_avg_sq", s))
    big = max(range(len(RAGGED)), key=RAGGED.__getitem__)
    assert v[big][0] == 0 and v[big][1] == 0 and 0 < v[big][3] < np.finfo(F).tiny
    p.tree.close()


def test_adamw_kernel_argument_errors_are_raised():
    tree = PackedTree([10, 20])
    s = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(tree.total, device=DEV)
    a = buf.data_ptr()
    sc = _sc(1)
    with pytest.raises(_lib.DilocoHipError, match="not bound"):
        _lib.call("dl_delta_pack_adamw", tree.handle, -1, SLOT_INNER, a, a, _lib.DL_F32, a, a,
                  *sc, s)
    with pytest.raises(_lib.DilocoHipError, match="not bound"):
        _lib.call("dl_unpack_adamw", tree.handle, -1, a, _lib.DL_F32, 1, a, a, a, *sc,
                  SLOT_INNER, s)
    tree.bind(SLOT_INNER, [torch.zeros(10, device=DEV), torch.zeros(20, device=DEV)], s)
    for args, msg in [((None, _lib.DL_F32, 1, a, a, a), "wire is null"),
                      ((a, _lib.DL_F32, 1, None, a, a), "outer is null"),
                      ((a, _lib.DL_F32, 1, a, None, a), "exp_avg is null"),
                      ((a, _lib.DL_F32, 1, a, a, None), "exp_avg_sq is null"),
                      ((a, 7, 1, a, a, a), "wire dtype"),
                      ((a, _lib.DL_F32, 0, a, a, a), "divisor"),
                      ((a, _lib.DL_F32, 1, a, a + 4, a), "aligned")]:
        with pytest.raises(_lib.DilocoHipError, match=msg):
            _lib.call("dl_unpack_adamw", tree.handle, -1, *args, *sc, SLOT_INNER, s)
    for args, msg in [((None, a, _lib.DL_F32, a, a), "outer is null"),
                      ((a, None, _lib.DL_F32, a, a), "wire is null"),
                      ((a, a, _lib.DL_F32, None, a), "exp_avg is null"),
                      ((a, a, _lib.DL_F32, a, None), "exp_avg_sq is null"),
                      ((a, a, _lib.DL_F16, a, a), "wire dtype"),
                      ((a, a + 8, _lib.DL_F32, a, a), "aligned")]:
        with pytest.raises(_lib.DilocoHipError, match=msg):
            _lib.call("dl_delta_pack_adamw", tree.handle, -1, SLOT_INNER, *args, *sc, s)
    with pytest.raises(_lib.DilocoHipError, match="bucket"):
        _lib.call("dl_unpack_adamw", tree.handle, 5, a, _lib.DL_F32, 1, a, a, a, *sc, -1, s)
    with pytest.raises(_lib.DilocoHipError, match="null tree"):
        _lib.call("dl_unpack_adamw", None, -1, a, _lib.DL_F32, 1, a, a, a, *sc, -1, s)
    torch.cuda.synchronize()
    assert not buf.any()  # nothing was launched
    tree.close()


# ---- the drop-in surface -------------------------------------------------------------------
class _Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


ADAMW_CFG = _Cfg(type="AdamW", **HYPER)


def _flat(ts):
    return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in ts])


def _module(values, shapes, device):
    m = torch.nn.Module()
    m.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(v.copy()).view(s))
                                   for v, s in zip(values, shapes)])
    return m.to(device)


def _dropin_steps(rank, world, device_placement, steps=3):
    """The reference's four calls with the fused AdamW outer optimizer on the micro tree in
    several buckets (this process = DP rank `rank` of `world`); beside them the restatement on
    every rank's inner values. At N = 2 on the device placement rank 0 alone reads .grad
    between sync_gradients and the step: local under the replicated exchange."""
    from diloco_amd.comm import TrainingComm
    from diloco_amd.optim import OuterAdamW
    from diloco_amd.utils import get_optimizer, get_outer_model
    from diloco_amd.world import World

    spec = get_tree("micro")
    shapes = [s for _, s in spec.params()]
    theta0 = synth.outer_tree(spec.numels(), spec.init_spec())
    inner = _module(theta0, shapes, "cpu")
    outer = get_outer_model(inner, "device" if device_placement else None)
    inner = inner.to(DEV)
    opt = get_optimizer(outer, ADAMW_CFG)
    assert type(opt) is OuterAdamW
    comm = TrainingComm(World.from_default_group(1), (1, 1, 32), None)
    ref = AdamWState(theta0, **HYPER)
    launches = []
    for name in ("delta_pack_adamw", "unpack_adamw"):  # record every launch of the two kernels
        def spy(*a, _f=getattr(K, name), _n=name):
            launches.append(_n)
            return _f(*a)
        setattr(K, name, spy)
    set_default_kernels(K)
    try:
        rec = _dropin_loop(rank, world, device_placement, steps, inner, outer, opt, comm, ref)
    finally:
        set_default_kernels(None)
        for name in ("delta_pack_adamw", "unpack_adamw"):
            delattr(K, name)  # the spies were instance attributes over the class's methods
    rec["launches"] = np.array(launches)
    rec["n_buckets"] = np.int64(outer._diloco_mirror.tree.n_buckets)
    return rec


def _dropin_loop(rank, world, device_placement, steps, inner, outer, opt, comm, ref):
    from diloco_amd.utils import compute_pseudo_gradient, sync_inner_model

    rec = {}
    for s in range(1, steps + 1):
        vals = [synth.inner_tree(ref.theta, s, r) for r in range(world)]
        with torch.no_grad():
            for p, v in zip(inner.parameters(), vals[rank]):
                p.copy_(torch.from_numpy(v).view(p.shape))
        compute_pseudo_gradient(inner, outer)
        comm.sync_gradients(outer)
        if world > 1 and device_placement and rank == 0 and s == 2:
            rec["lone_grad"] = _flat(p.grad for p in outer.parameters())  # must not raise
        opt.step()
        sync_inner_model(outer, inner)
        _, avg = ref.step(vals)
        torch.cuda.synchronize()
        st = [opt.state[p] for p in outer.parameters()]
        rec[f"theta_s{s}"] = _flat(outer.parameters())
        rec[f"inner_s{s}"] = _flat(inner.parameters())
        rec[f"avg_s{s}"] = _flat(p.grad for p in outer.parameters())
        rec[f"exp_avg_s{s}"] = _flat(x["exp_avg"] for x in st)
        rec[f"exp_avg_sq_s{s}"] = _flat(x["exp_avg_sq"] for x in st)
        rec[f"step_s{s}"] = np.array([float(x["step"]) for x in st])
        rec[f"ref_theta_s{s}"] = np.concatenate(ref.theta)
        rec[f"ref_avg_s{s}"] = np.concatenate(avg)
        rec[f"ref_exp_avg_s{s}"] = np.concatenate(ref.m)
        rec[f"ref_exp_avg_sq_s{s}"] = np.concatenate(ref.v)
    return rec


def _check_dropin(rec, steps=3):
    for s in range(1, steps + 1):
        assert rec[f"inner_s{s}"].tobytes() == rec[f"theta_s{s}"].tobytes(), s
        for key in ("theta", "avg", "exp_avg", "exp_avg_sq"):
            got, want = rec[f"{key}_s{s}"], rec[f"ref_{key}_s{s}"]
            assert got.tobytes() == want.tobytes(), (key, s, int((got != want).sum()))
        assert (rec[f"step_s{s}"] == s).all()


@pytest.mark.parametrize("placement", ["host", "device"])
def test_dropin_fused_adamw_one_peer(placement, monkeypatch):
    """One peer, both placements: every outer step is ONE dl_delta_pack_adamw, and θ, the inner
    params, .grad, exp_avg and exp_avg_sq equal the restatement bit for bit."""
    monkeypatch.setenv("DILOCO_OUTER_ADAMW", "fused")
    monkeypatch.setenv("DILOCO_OUTER_BUCKET_ELEMS", "4096")
    made = not dist.is_initialized()
    if made:
        f = tempfile.mktemp(prefix="dl_pg_")
        dist.init_process_group("gloo", init_method=f"file://{f}", rank=0, world_size=1)
    try:
        rec = _dropin_steps(0, 1, placement == "device")
    finally:
        if made:  # later tests emulate a peer in-process and expect no job's process group
            dist.destroy_process_group()
    _check_dropin(rec)
    assert list(rec["launches"]) == ["delta_pack_adamw"] * 3


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, device_placement, out):
    for p in (PKG, REPO, os.path.join(REPO, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["DILOCO_DP_BACKEND"] = "gloo"
    os.environ["DILOCO_OUTER_ADAMW"] = "fused"
    os.environ["DILOCO_OUTER_BUCKET_ELEMS"] = "4096"
    os.environ.pop("DILOCO_OUTER_EXCHANGE", None)
    # a .grad read that turned out to be a collective fails fast instead of waiting
    os.environ["DILOCO_COLLECTIVE_READ_TIMEOUT"] = "10"
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank,
                            world_size=world)
    rec = _dropin_steps(rank, world, device_placement)
    np.savez(os.path.join(out, f"r{rank}.npz"), **rec)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("placement", ["host", "device"])
def test_dropin_fused_adamw_two_peers(placement):
    """Two gloo processes on the GPU, several buckets: pack -> all_reduce -> dl_unpack_adamw
    per bucket with the /2 in the divisor. (d0 + d1) / 2 is order-independent, so θ, inner,
    .grad, exp_avg and exp_avg_sq equal the restatement bit for bit on both ranks. On the
    device placement rank 0 alone reads .grad mid-sequence without raising: the exchange is the
    replicated one, not that placement's implicit sharded default."""
    out = tempfile.mkdtemp(prefix="dl_adamw_")
    mp.spawn(_worker, args=(2, _free_port(), placement == "device", out), nprocs=2, join=True)
    recs = [dict(np.load(os.path.join(out, f"r{r}.npz"))) for r in range(2)]
    for r, rec in enumerate(recs):
        _check_dropin(rec)
        nb = int(rec["n_buckets"])
        assert nb > 2
        want = ["unpack_adamw"] * (3 * nb)
        if placement == "device" and r == 0:  # the lone .grad read joined step 2's buckets
            want = ["unpack_adamw"] * (2 * nb + 1)
            assert rec["lone_grad"].tobytes() == rec["ref_avg_s2"].tobytes()
        assert list(rec["launches"]) == want, r
