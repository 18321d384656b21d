"""The fused AdamW outer step on the int8 wire, on the GPU: dl_unpack_adamw_q8 against the
numpy restatement of its contract (g = float(int8 q) * s, then tests/adamw_restatement.py) on
the ragged tree, against its two-kernel equivalent (the decoded values through dl_unpack_adamw),
with IEEE special values in the scales, and the reference's four calls with
DILOCO_OUTER_ADAMW=fused and wire="int8" over two gloo processes on the one GPU (RCCL refuses
two ranks on one device; the kernels are the product's)."""
import os
import socket
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from adamw_restatement import AdamWState, F, adamw_elementwise, scalars
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
# tests/test_kernels_gpu.py's ragged tree: an empty tensor, tails under 4, chunk edges, a
# 1-element chunk and (bucket cap 4096) several buckets
RAGGED = [1, 3, 5, 4097, 0, 64, 65, 12345, 8191, 4096 * 3 + 7, 2]
CAP = 4096
SLOT, HDR = oracle.Q8_SLOT, oracle.Q8_HDR
K = HipKernels()
# (tensor, offset in it, length) of every chunk, in tree order: the slot order
CHUNKS = [(t, o, n) for t, numel in enumerate(RAGGED) for o, n in oracle.chunks_of(numel)]


def _sc(t):
    return adamw_scalars(HYPER["lr"], *HYPER["betas"], HYPER["weight_decay"], EPS, float(t))


def _ref_sc(t):
    return scalars(HYPER["lr"], HYPER["betas"], HYPER["weight_decay"], EPS, t)


def _inner_tensors(host, misaligned):
    """Per-tensor device storage: separate allocations, or slices of one buffer at odd element
    offsets (4-B aligned only: the kernel's element-wise path)."""
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
    """θ, exp_avg, exp_avg_sq, an fp32 wire and the tree's int8 slots (one per chunk, in chunk
    order, no padding slots) in a PackedTree's layout.
    Its padding checks use zero as the sentinel; tests/test_footprint_gpu.py pins the footprint."""

    def __init__(self, theta, inner0=None, misaligned=False):
        self.tree = PackedTree(RAGGED, CAP)
        assert self.tree.n_buckets > 2 and self.tree.n_chunks == len(CHUNKS)
        z = dict(dtype=torch.float32, device=DEV)
        self.theta = torch.zeros(self.tree.total, **z)
        self.m = torch.zeros(self.tree.total, **z)
        self.v = torch.zeros(self.tree.total, **z)
        self.wire = torch.zeros(self.tree.total, **z)
        self.slots = torch.zeros(len(CHUNKS) * SLOT, dtype=torch.uint8, device=DEV)
        self.offs = [int(o) for o in self.tree.seg_off[:-1]]
        self.put(self.theta, theta)
        self.inner = None
        if inner0 is not None:
            self.inner = _inner_tensors(inner0, misaligned)
            self.tree.bind(SLOT_INNER, self.inner, torch.cuda.current_stream().cuda_stream)

    def put(self, buf, host):
        for o, h in zip(self.offs, host):
            buf[o:o + h.size].copy_(torch.from_numpy(np.ascontiguousarray(h)))

    def get(self, buf):
        b = buf.cpu().numpy()
        return [b[o:o + n].copy() for o, n in zip(self.offs, RAGGED)]

    def bucket_slots(self, b):
        """The slots of bucket b: its first chunk's slot at offset 0 (16-B aligned: 4160 is)."""
        c0, c1 = self.tree.bucket_chunks[b]
        return self.slots[c0 * SLOT:c1 * SLOT]

    def step_q8(self, s, slot, whole=False):
        if whole:
            K.unpack_adamw_q8(self.tree, _lib.ALL_BUCKETS, self.slots, self.theta, self.m, self.v,
                              _sc(s), slot)
            return
        for b in range(self.tree.n_buckets):
            K.unpack_adamw_q8(self.tree, b, self.bucket_slots(b), self.theta, self.m, self.v,
                              _sc(s), slot)

    def padding_is_zero(self, *bufs):
        mask = torch.ones(self.tree.total, dtype=torch.bool, device=DEV)
        for o, n in zip(self.offs, RAGGED):
            mask[o:o + n] = False
        return not any(bool(b[mask].any()) for b in bufs)


def _eq(got, want, what):
    for t, (a, b) in enumerate(zip(got, want)):
        assert a.tobytes() == b.tobytes(), (what, t, int((a != b).sum()))


def _same(got, want, what):
    """NaNs by position (payloads are not part of the contract), every other value by its bytes."""
    for t, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(np.isnan(a), np.isnan(b)), (what, t, "NaN positions")
        ok = ~np.isnan(b)
        assert a[ok].tobytes() == b[ok].tobytes(), (what, t)


def _slots(rng, scale_of=None):
    """Host slots of the whole tree and the values they decode to, per tensor. Payload: int8 in
    [-127, 127] with both ends present and runs of zeros; the scale of chunk c is scale_of(c)
    when that gives one, else positive over six decades with every fifth chunk exactly 0; bytes
    past a chunk's length and the header past the scale stay zero."""
    raw = np.zeros(len(CHUNKS) * SLOT, np.uint8)
    g = [np.zeros(n, F) for n in RAGGED]
    for c, (t, o, n) in enumerate(CHUNKS):
        q = rng.integers(-127, 128, n).astype(np.int8)
        q[::7] = 127
        q[3::7] = -127
        q[n // 3:n // 3 + max(1, n // 8)] = 0
        s = scale_of(c) if scale_of is not None else None
        if s is None:
            s = F(0) if c % 5 == 2 else F(10.0 ** rng.uniform(-6, 0))
        s = F(s)
        at = c * SLOT
        raw[at:at + 4] = np.array([s], F).view(np.uint8)
        raw[at + HDR:at + HDR + n] = q.view(np.uint8)
        with np.errstate(all="ignore"):
            g[t][o:o + n] = q.astype(F) * s  # one rounded fp32 multiply
    return raw, g


@pytest.mark.parametrize("inner", ["aligned", "misaligned", "unbound"])
def test_unpack_adamw_q8_matches_the_restatement(inner):
    """dl_unpack_adamw_q8 bucket by bucket on the ragged tree, three steps from a zero state: θ,
    exp_avg, exp_avg_sq and the inner tensors (inner_slot -1: untouched) bit-equal to the
    restatement on g = q.astype(f32) * s; the slots are only read; padding stays zero."""
    rng = np.random.default_rng(41)
    th = [rng.standard_normal(n).astype(F) for n in RAGGED]
    m = [np.zeros(n, F) for n in RAGGED]
    v = [np.zeros(n, F) for n in RAGGED]
    inner0 = [rng.standard_normal(n).astype(F) for n in RAGGED]
    p = _Packed(th, inner0, inner == "misaligned")
    slot = -1 if inner == "unbound" else SLOT_INNER
    for s in (1, 2, 3):
        raw, g = _slots(rng)
        p.slots.copy_(torch.from_numpy(raw))
        p.step_q8(s, slot)
        torch.cuda.synchronize()
        for t in range(len(RAGGED)):
            th[t], m[t], v[t] = adamw_elementwise(th[t], m[t], v[t], g[t], _ref_sc(s))
        _eq(p.get(p.theta), th, ("theta", s))
        _eq(p.get(p.m), m, ("exp_avg", s))
        _eq(p.get(p.v), v, ("exp_avg_sq", s))
        _eq([x.cpu().numpy() for x in p.inner], inner0 if inner == "unbound" else th,
            ("inner", s))
        assert p.slots.cpu().numpy().tobytes() == raw.tobytes(), s
        assert p.padding_is_zero(p.theta, p.m, p.v)
    p.tree.close()


@pytest.mark.parametrize("misaligned", [False, True])
def test_unpack_adamw_q8_equals_decode_then_unpack_adamw(misaligned):
    """The same slots three ways on three sets of buffers: dl_unpack_adamw_q8 per bucket, one
    whole-tree launch of it (DL_ALL_BUCKETS: every slot in chunk order, no padding slots), and
    dl_unpack_adamw (fp32 wire, divisor 1) on the decoded values. θ, exp_avg, exp_avg_sq and
    inner byte-equal after each of three steps."""
    rng = np.random.default_rng(43)
    theta0 = [rng.standard_normal(n).astype(F) for n in RAGGED]
    inner0 = [rng.standard_normal(n).astype(F) for n in RAGGED]
    one, all_, two = (_Packed(theta0, inner0, misaligned) for _ in range(3))
    for s in (1, 2, 3):
        raw, g = _slots(rng)
        for p in (one, all_):
            p.slots.copy_(torch.from_numpy(raw))
        two.put(two.wire, g)
        one.step_q8(s, SLOT_INNER)
        all_.step_q8(s, SLOT_INNER, whole=True)
        for b in range(two.tree.n_buckets):
            K.unpack_adamw(two.tree, b, two.wire, 1, two.theta, two.m, two.v, _sc(s), SLOT_INNER)
        torch.cuda.synchronize()
        for p in (one, all_):
            for name in ("theta", "m", "v"):
                assert torch.equal(getattr(p, name), getattr(two, name)), (name, s)
            for t, (a, b) in enumerate(zip(p.inner, two.inner)):
                assert torch.equal(a, b), ("inner", s, t)
    assert bool(one.theta.ne(torch.cat([torch.from_numpy(x) for x in theta0]).to(DEV)[0]).any())
    for p in (one, all_, two):
        p.tree.close()


@pytest.mark.parametrize("misaligned", [False, True])
def test_unpack_adamw_q8_special_values(misaligned):
    """Scale +inf in one slot (g = ±inf, and NaN where q = 0), NaN in another, a denormal scale
    (g denormal: the library keeps denormals, g*g underflows) and an exactly-zero scale on the
    zero state (v = 0, g = 0: den = eps), each in a full chunk and in a short one, three steps:
    bit-equal to the restatement with NaNs compared by position, so the chunks beside them are
    unaffected."""
    big = [c for c, (t, o, n) in enumerate(CHUNKS) if n == 4096]
    short = [c for c, (t, o, n) in enumerate(CHUNKS) if n < 4096]
    # 127 * 9e-41 < FLT_MIN: every g of a denormal-scale chunk is itself denormal
    special = {big[0]: np.inf, big[2]: np.nan, big[4]: 9e-41, big[5]: 0.0,
               short[0]: np.nan, short[2]: np.inf, short[4]: 0.0, short[6]: 3e-41}

    rng = np.random.default_rng(47)
    th = [rng.standard_normal(n).astype(F) for n in RAGGED]
    m = [np.zeros(n, F) for n in RAGGED]
    v = [np.zeros(n, F) for n in RAGGED]
    p = _Packed(th, th, misaligned)
    raw, g = _slots(rng, special.get)
    p.slots.copy_(torch.from_numpy(raw))
    for s in (1, 2, 3):
        p.step_q8(s, SLOT_INNER)
        torch.cuda.synchronize()
        for t in range(len(RAGGED)):
            th[t], m[t], v[t] = adamw_elementwise(th[t], m[t], v[t], g[t], _ref_sc(s))
        _same(p.get(p.theta), th, ("theta", s))
        _same(p.get(p.m), m, ("exp_avg", s))
        _same(p.get(p.v), v, ("exp_avg_sq", s))
        _same([x.cpu().numpy() for x in p.inner], th, ("inner", s))
        assert p.padding_is_zero(p.theta, p.m, p.v)
    # the planted cases are what they claim to be, and the other chunks stayed finite
    for c, (t, o, n) in enumerate(CHUNKS):
        sl = slice(o, o + n)
        if c not in special:
            assert np.isfinite(th[t][sl]).all() and np.isfinite(v[t][sl]).all(), c
        elif special[c] == 0.0:
            assert not v[t][sl].any() and not m[t][sl].any(), c
        elif np.isfinite(special[c]):
            assert not v[t][sl].any() and m[t][sl].any(), c  # g*g underflows, g does not
            assert (np.abs(g[t][sl]) < np.finfo(F).tiny).all(), c
        else:
            assert np.isnan(th[t][sl]).all(), c
    p.tree.close()


def test_unpack_adamw_q8_argument_errors_are_raised():
    tree = PackedTree([10, 20])
    s = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(2 * SLOT, device=DEV)
    a = buf.data_ptr()
    sc = _sc(1)
    with pytest.raises(_lib.DilocoHipError, match="not bound"):
        _lib.call("dl_unpack_adamw_q8", tree.handle, -1, a, a, a, a, *sc, SLOT_INNER, s)
    for args, msg in [((None, a, a, a), "slots is null"), ((a, None, a, a), "outer is null"),
                      ((a, a, None, a), "exp_avg is null"), ((a, a, a, None), "exp_avg_sq is null"),
                      ((a + 4, a, a, a), "aligned"), ((a, a, a + 8, a), "aligned")]:
        with pytest.raises(_lib.DilocoHipError, match=msg):
            _lib.call("dl_unpack_adamw_q8", tree.handle, -1, *args, *sc, -1, s)
    with pytest.raises(_lib.DilocoHipError, match="bucket"):
        _lib.call("dl_unpack_adamw_q8", tree.handle, 5, a, a, a, a, *sc, -1, s)
    torch.cuda.synchronize()
    assert not buf.any()  # nothing was launched
    tree.close()


# ---- the drop-in surface -------------------------------------------------------------------
class _Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


KEYS = ("theta", "inner", "grad", "exp_avg", "exp_avg_sq")
STEPS = 3


def _flat(ts):
    return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in ts])


def _dropin(rank, world, device_placement, read_every_step):
    """The reference's four calls with the fused AdamW outer optimizer on the int8 wire, micro
    tree in three or more buckets (this process = DP rank `rank` of `world`); beside them the
    restatement on the oracle's int8 exchange. read_every_step: θ, inner, .grad and the state
    are read after every step; otherwise nothing is read until the last step is done."""
    from diloco_amd.comm import TrainingComm
    from diloco_amd.optim import OuterAdamW
    from diloco_amd.utils import (compute_pseudo_gradient, get_optimizer, get_outer_model,
                                  outer_mirror, sync_inner_model)
    from diloco_amd.world import World

    spec = get_tree("micro")
    numels = spec.numels()
    shapes = [s for _, s in spec.params()]
    theta0 = synth.outer_tree(numels, spec.init_spec())
    inner = torch.nn.Module()
    inner.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(v.copy()).view(s))
                                       for v, s in zip(theta0, shapes)])
    outer = get_outer_model(inner, "device" if device_placement else None, wire="int8")
    inner = inner.to(DEV)
    opt = get_optimizer(outer, _Cfg(type="AdamW", **HYPER))
    assert type(opt) is OuterAdamW
    comm = TrainingComm(World.from_default_group(1), (1, 1, 32), None)
    ref = AdamWState(theta0, **HYPER)
    rec, counts = {}, None

    def read(s, avg):
        st = [opt.state[p] for p in outer.parameters()]
        rec[f"theta_s{s}"] = _flat(outer.parameters())
        rec[f"inner_s{s}"] = _flat(inner.parameters())
        rec[f"grad_s{s}"] = _flat(p.grad for p in outer.parameters())
        rec[f"exp_avg_s{s}"] = _flat(x["exp_avg"] for x in st)
        rec[f"exp_avg_sq_s{s}"] = _flat(x["exp_avg_sq"] for x in st)
        rec[f"step_s{s}"] = np.array([float(x["step"]) for x in st])
        rec[f"ref_theta_s{s}"] = rec[f"ref_inner_s{s}"] = np.concatenate(ref.theta)
        rec[f"ref_grad_s{s}"] = np.concatenate(avg)
        rec[f"ref_exp_avg_s{s}"] = np.concatenate(ref.m)
        rec[f"ref_exp_avg_sq_s{s}"] = np.concatenate(ref.v)

    for s in range(1, STEPS + 1):
        vals = [synth.inner_tree(ref.theta, s, r) for r in range(world)]
        with torch.no_grad():
            for p, v in zip(inner.parameters(), vals[rank]):
                p.copy_(torch.from_numpy(v).view(p.shape))
        compute_pseudo_gradient(inner, outer)
        comm.sync_gradients(outer)
        opt.step()
        sync_inner_model(outer, inner)
        if counts is None:  # the device placement's mirror exists from the first delta on
            m = outer_mirror(outer)
            tree = getattr(m, "dev", m).tree
            counts = [c1 - c0 for c0, c1 in tree.bucket_chunks]
            rec["n_buckets"] = np.int64(tree.n_buckets)
        deltas = [[oracle.delta(t, i) for t, i in zip(ref.theta, v)] for v in vals]
        avg = oracle.q8_average(deltas, numels, counts)
        ref.step_grads(avg)
        if read_every_step or s == STEPS:
            torch.cuda.synchronize()
            read(s, avg)
    return rec


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, device_placement, out):
    for p in (PKG, REPO, os.path.join(REPO, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import expect

    os.environ["DILOCO_DP_BACKEND"] = "gloo"
    os.environ["DILOCO_OUTER_ADAMW"] = "fused"
    os.environ["DILOCO_OUTER_BUCKET_ELEMS"] = str(expect.MICRO_Q8_CAP)
    for v in ("DILOCO_OUTER_EXCHANGE", "DILOCO_DP_EXCHANGE", "DILOCO_OUTER_WIRE",
              "DILOCO_OUTER_FUSED"):
        os.environ.pop(v, None)
    # a .grad read that turned out to be a collective fails fast instead of waiting
    os.environ["DILOCO_COLLECTIVE_READ_TIMEOUT"] = "10"
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank,
                            world_size=world)
    launches = []
    names = ("unpack_adamw_q8", "unpack_adamw", "delta_pack_adamw")
    for name in names:  # record every launch of the AdamW kernels
        def spy(*a, _f=getattr(K, name), _n=name):
            launches.append(_n)
            return _f(*a)
        setattr(K, name, spy)
    set_default_kernels(K)
    try:
        for mode, every in (("quiet", False), ("read", True)):
            n0 = len(launches)
            rec = _dropin(rank, world, device_placement, every)
            rec["launches"] = np.array(launches[n0:])
            np.savez(os.path.join(out, f"{mode}_r{rank}.npz"), **rec)
    finally:
        set_default_kernels(None)
        for name in names:
            delattr(K, name)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("placement", ["host", "device"])
def test_dropin_int8_wire_adamw_two_peers_on_gpu(placement):
    """Two gloo processes on the GPU, three or more buckets: dl_delta_q8 -> all_to_all ->
    dl_q8_reduce -> all_gather -> dl_unpack_adamw_q8 per bucket. The int8 exchange sums in rank
    order, so θ, inner, .grad (decoded from the slots after the step), exp_avg and exp_avg_sq
    equal the restatement bit for bit on both ranks -- with nothing read until the last step is
    done, and with everything read after every step."""
    out = tempfile.mkdtemp(prefix="dl_q8_adamw_")
    mp.spawn(_worker, args=(2, _free_port(), placement == "device", out), nprocs=2, join=True)
    for mode in ("quiet", "read"):
        recs = [dict(np.load(os.path.join(out, f"{mode}_r{r}.npz"))) for r in range(2)]
        for rec in recs:
            nb = int(rec["n_buckets"])
            assert nb >= 3
            assert list(rec["launches"]) == ["unpack_adamw_q8"] * (STEPS * nb), mode
            for s in range(1 if mode == "read" else STEPS, STEPS + 1):
                for key in KEYS:
                    got, want = rec[f"{key}_s{s}"], rec[f"ref_{key}_s{s}"]
                    assert got.tobytes() == want.tobytes(), (mode, key, s, int((got != want).sum()))
                    assert got.tobytes() == recs[0][f"{key}_s{s}"].tobytes(), (mode, key, s)
                assert (rec[f"step_s{s}"] == s).all()
