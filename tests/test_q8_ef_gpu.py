"""Error feedback on the int8 wire, on the GPU: dl_delta_q8_ef and dl_q8_reduce_ef against the
numpy restatement (tests/q8_ef_restatement.py, walked over the packed layout by
tests/q8_ef_oracle_kernels.py), bit for bit, NaNs by position.

The tree has a 1-element chunk, tails under 4, a chunk one short of full, a full one, one that
spills a single element into a second chunk, and a three-chunk tensor; bucket cap 4096 splits it
into several buckets. Inner tensors sit in their own allocations (16-B aligned: the vector
path) or one float off (the scalar path)."""
import os
import socket
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import q8_ef_restatement as ef
from conftest import PKG, REPO
from diloco_amd import _lib, synth
from diloco_amd.kernels import HipKernels, set_default_kernels
from diloco_amd.outer import OuterSync
from diloco_amd.plan import SLOT_INNER, PackedTree
from diloco_amd.trees import get_tree
from oracle import oracle
from oracle_kernels import CpuTree
from q8_ef_oracle_kernels import Q8EFOracleKernels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
NUMELS = [1, 3, 257, 4095, 4096, 4097, 8197]
CAP = 4096
SLOT, HDR, CHUNK = oracle.Q8_SLOT, oracle.Q8_HDR, oracle.CHUNK
ALL = _lib.ALL_BUCKETS
SENTINEL = 0x7F8BEEF5  # a NaN bit pattern: the residual arena's padding before every run
K = HipKernels()
REF = Q8EFOracleKernels()


def _pseudo_gradient_tree(rng):
    """θ and inner whose difference has one element of ~1 per chunk-sized stretch and ~1e-3
    elsewhere: most elements quantise to 0 and live on in the residual."""
    theta = [rng.standard_normal(n).astype(F) for n in NUMELS]
    inner = []
    for t in theta:
        d = (1e-3 * rng.standard_normal(t.size)).astype(F)
        d[::1500] = 1.0
        inner.append((t - d).astype(F))
    return theta, inner


class _Rig:
    """One tree on the device (θ, residual, slots, inner tensors) and its host twin on the
    checker backend, fed the same values.
    Only the residual's padding holds a sentinel here; tests/test_footprint_gpu.py pins the footprint."""

    def __init__(self, misaligned=False, max_blocks=0):
        self.tree = PackedTree(NUMELS, CAP)
        self.cpu = CpuTree(NUMELS, CAP)
        assert self.tree.n_buckets >= 2 and self.tree.bucket_chunks == self.cpu.bucket_chunks
        assert self.tree.total == self.cpu.total
        if max_blocks:
            self.tree.tune(max_blocks)
        self.offs = [int(o) for o in self.tree.seg_off[:-1]]
        self.pad = np.ones(self.tree.total, dtype=bool)
        for o, n in zip(self.offs, NUMELS):
            self.pad[o:o + n] = False
        z = dict(dtype=torch.float32, device=DEV)
        self.theta = torch.zeros(self.tree.total, **z)
        res0 = np.zeros(self.tree.total, dtype=np.uint32)
        res0[self.pad] = SENTINEL
        self.resid = torch.from_numpy(res0.view(F).copy()).to(DEV)
        self.slots = torch.zeros(self.tree.n_chunks * SLOT, dtype=torch.uint8, device=DEV)
        if misaligned:
            base = torch.zeros(sum(NUMELS) + 8 * len(NUMELS) + 8, **z)
            self.inner, at = [], 1
            for n in NUMELS:
                self.inner.append(base[at:at + n])
                assert self.inner[-1].data_ptr() % 16 == 4
                at += n + (-n) % 4 + 4
        else:
            self.inner = [torch.zeros(n, **z) for n in NUMELS]
            assert all(t.data_ptr() % 16 == 0 for t in self.inner)
        self.tree.bind(SLOT_INNER, self.inner, torch.cuda.current_stream().cuda_stream)
        self.h_theta = torch.zeros(self.tree.total)
        self.h_resid = torch.from_numpy(res0.view(F).copy())
        self.h_slots = torch.zeros(self.tree.n_chunks * SLOT, dtype=torch.uint8)
        self.h_inner = [torch.zeros(n) for n in NUMELS]
        REF.bind(self.cpu, SLOT_INNER, self.h_inner, None)

    def feed(self, theta, inner, resid=None):
        for o, t, i, d, h in zip(self.offs, theta, inner, self.inner, self.h_inner):
            self.h_theta[o:o + t.size] = torch.from_numpy(t)
            h.copy_(torch.from_numpy(i))
            d.copy_(h)
        self.theta.copy_(self.h_theta)
        if resid is not None:
            for o, r in zip(self.offs, resid):
                self.h_resid[o:o + r.size] = torch.from_numpy(r)
            self.resid.copy_(self.h_resid)

    def bucket_slots(self, buf, b):
        c0, c1 = self.tree.bucket_chunks[b]
        return buf[c0 * SLOT:c1 * SLOT]

    def encode(self, whole=False, reference=True):
        if whole:
            K.delta_q8_ef(self.tree, ALL, SLOT_INNER, self.theta, self.resid, self.slots)
        else:
            for b in range(self.tree.n_buckets):
                K.delta_q8_ef(self.tree, b, SLOT_INNER, self.theta, self.resid,
                              self.bucket_slots(self.slots, b))
        if reference:
            REF.delta_q8_ef(self.cpu, ALL, SLOT_INNER, self.h_theta, self.h_resid, self.h_slots)
        torch.cuda.synchronize()

    def check(self, what):
        got_s, want_s = self.slots.cpu().numpy(), self.h_slots.numpy()
        assert got_s.tobytes() == want_s.tobytes(), (what, "slots",
                                                     int((got_s != want_s).sum()))
        got_r, want_r = self.resid.cpu().numpy(), self.h_resid.numpy()
        assert ef.same_bits(got_r[~self.pad], want_r[~self.pad]), (what, "residual")
        # the residual arena's padding is never written; slot bytes past a chunk stay zero
        assert (got_r.view(np.uint32)[self.pad] == SENTINEL).all(), (what, "padding")
        for c, (_seg, _o, n, _po) in enumerate(self.cpu.chunks):
            assert not got_s[c * SLOT + HDR + n:(c + 1) * SLOT].any(), (what, "slot tail", c)
            assert not got_s[c * SLOT + 4:c * SLOT + HDR].any(), (what, "header", c)


@pytest.mark.parametrize("misaligned", [False, True])
def test_delta_q8_ef_matches_the_restatement(misaligned):
    """Three consecutive steps, bucket by bucket: the residual of one step feeds the next."""
    rng = np.random.default_rng(61)
    rig = _Rig(misaligned)
    for s in (1, 2, 3):
        rig.feed(*_pseudo_gradient_tree(rng))
        rig.encode()
        rig.check(s)
        r = rig.resid.cpu().numpy()[~rig.pad]
        assert np.isfinite(r).all() and r.any()
    rig.tree.close()


@pytest.mark.parametrize("misaligned", [False, True])
def test_delta_q8_ef_does_not_depend_on_the_launch_shape(misaligned):
    """Per bucket, one whole-tree launch, and two workgroups walking all the chunks (the LDS
    stage and the amax partials are reused chunk after chunk): the same bytes, two steps."""
    rng = np.random.default_rng(67)
    rigs = [_Rig(misaligned), _Rig(misaligned), _Rig(misaligned, max_blocks=2)]
    for s in (1, 2):
        theta, inner = _pseudo_gradient_tree(rng)
        for i, rig in enumerate(rigs):
            rig.feed(theta, inner)
            rig.encode(whole=i > 0, reference=i == 0)
        rigs[0].check(s)
        for rig in rigs[1:]:
            assert torch.equal(rig.slots, rigs[0].slots), s
            assert torch.equal(rig.resid.view(torch.int32), rigs[0].resid.view(torch.int32)), s
    for rig in rigs:
        rig.tree.close()


def test_zero_residual_gives_the_plain_encoders_slots():
    rng = np.random.default_rng(71)
    rig = _Rig()
    rig.feed(*_pseudo_gradient_tree(rng))
    plain = torch.zeros_like(rig.slots)
    K.delta_q8(rig.tree, ALL, SLOT_INNER, rig.theta, plain)
    rig.encode(whole=True, reference=False)
    assert torch.equal(rig.slots, plain)
    rig.tree.close()


MAXF = float(np.finfo(F).max)
# (θ, inner, residual) triples: NaN, ±Inf, ±0, subnormals, ±FLT_MAX whose difference overflows
WILD = [(np.nan, 1.0, 0.0), (np.inf, 1.0, 0.0), (-np.inf, np.inf, 0.0), (1.0, 1.0, np.inf),
        (MAXF, -MAXF, 0.0), (-MAXF, MAXF, 1.0), (1.0, 0.0, np.nan), (0.0, 0.0, -np.inf)]
TAME = [(0.0, -0.0, 0.0), (-0.0, 0.0, -0.0), (-0.0, -0.0, -0.0), (1e-40, 2e-40, 0.0),
        (0.0, 0.0, 1e-40), (5e-39, -5e-39, -3e-41), (1e-38, 1.1e-38, 1e-45), (1e-30, 1e-30, 0.0)]


@pytest.mark.parametrize("misaligned", [False, True])
def test_delta_q8_ef_special_values(misaligned):
    """One step. Chunks with an Inf or an overflowing difference get s = Inf (every residual of
    the chunk becomes NaN or Inf, by IEEE rules); a chunk whose only oddity is NaN keeps a
    finite scale (fmaxf ignores the NaN) and NaN residuals exactly where x is NaN; chunks of
    ±0 and subnormals only (denormals are kept: s itself is subnormal) stay finite."""
    rng = np.random.default_rng(73)
    theta = [(rng.standard_normal(n) * 0.02).astype(F) for n in NUMELS]
    inner = [(rng.standard_normal(n) * 0.02).astype(F) for n in NUMELS]
    resid = [(rng.standard_normal(n) * 1e-4).astype(F) for n in NUMELS]

    def plant(t, at, triples):
        for k, (a, b, c) in enumerate(triples):
            theta[t][at + k], inner[t][at + k], resid[t][at + k] = a, b, c

    plant(5, 0, WILD)  # chunk start of a full chunk
    plant(6, 4096 - 4, WILD)  # across a chunk boundary
    plant(6, 8197 - 3, [(np.nan, 0.0, 0.0), (1.0, np.nan, 0.0), (0.0, 0.0, np.nan)])  # the tail
    for t in (2, 3):  # finite oddities only, in chunks that hold nothing else
        theta[t][:], inner[t][:], resid[t][:] = 0.0, 0.0, 0.0
        plant(t, NUMELS[t] - len(TAME), TAME)
    rig = _Rig(misaligned)
    rig.feed(theta, inner, resid)
    rig.encode()
    rig.check("special")
    r = rig.resid.cpu().numpy()
    got = [r[o:o + n] for o, n in zip(rig.offs, NUMELS)]
    assert np.isfinite(got[2]).all() and np.isfinite(got[3]).all() and np.isfinite(got[4]).all()
    assert not np.isfinite(got[5][:4096]).any()  # s = Inf: 0 * Inf = NaN, Inf - (-Inf) = Inf
    tail = got[6][8192:]
    assert np.isnan(tail[2:]).all() and np.isfinite(tail[:2]).all()
    rig.tree.close()


def test_delta_q8_ef_argument_errors_are_raised():
    tree = PackedTree([10, 20])
    s = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(2 * SLOT, device=DEV)
    a = buf.data_ptr()
    with pytest.raises(_lib.DilocoHipError, match="not bound") as e:
        _lib.call("dl_delta_q8_ef", tree.handle, ALL, SLOT_INNER, a, a, a, s)
    assert e.value.code == -2 and "dl_delta_q8_ef" in str(e.value)  # DL_E_STATE
    tree.bind(SLOT_INNER, [torch.zeros(10, device=DEV), torch.zeros(20, device=DEV)], s)
    for args, msg in [((a, None, a), "residual is null"), ((a, a + 4, a), "residual not 16-B"),
                      ((None, a, a), "outer is null"), ((a, a, None), "slots is null"),
                      ((a, a, a + 8), "slots not 16-B")]:
        with pytest.raises(_lib.DilocoHipError, match=msg) as e:
            _lib.call("dl_delta_q8_ef", tree.handle, ALL, SLOT_INNER, *args, s)
        assert e.value.code == (-1 if "null" in msg else -3)  # DL_E_ARG / DL_E_ALIGN
    for args, msg in [((a, 1, 1, 1, None, a), "residual is null"),
                      ((a, 1, 1, 1, a + 4, a), "residual not 16-B"),
                      ((a, 2, 1, 2, a, a), "in place")]:
        with pytest.raises(_lib.DilocoHipError, match=msg):
            _lib.call("dl_q8_reduce_ef", *args, s)
    torch.cuda.synchronize()
    assert not buf.any()  # nothing was launched
    tree.close()


@pytest.mark.parametrize("n_peers", [1, 2, 3])
def test_q8_reduce_ef_matches_the_restatement(n_peers):
    """Three slots per peer -- a full chunk, a short one (zero tail) and an all-zero padding
    slot -- for two steps from a residual that is already nonzero where the slots hold values
    (one peer's own slots re-quantise exactly, so only a residual brought along shows there);
    at one peer in place, as the engine's one-replica reduce is."""
    rng = np.random.default_rng(79 + n_peers)
    m = 3
    res = np.zeros(m * CHUNK, dtype=F)
    res[:CHUNK + 1000] = (1e-3 * rng.standard_normal(CHUNK + 1000)).astype(F)
    d_res = torch.from_numpy(res).to(DEV)
    for s in (1, 2):
        recv = np.zeros(n_peers * m * SLOT, dtype=np.uint8)
        for r in range(n_peers):
            for j, n in enumerate((CHUNK, 1000)):
                x = (1e-3 * rng.standard_normal(n)).astype(F)
                x[rng.integers(n)] = 1.0 + r
                at = (r * m + j) * SLOT
                recv[at:at + SLOT] = oracle.delta_q8_from(x)
        want, res = ef.reduce_slots(recv, n_peers, m, n_peers, res)
        d_recv = torch.from_numpy(recv).to(DEV)
        d_out = d_recv if n_peers == 1 else torch.zeros(m * SLOT, dtype=torch.uint8, device=DEV)
        K.q8_reduce_ef(d_recv, n_peers, m, n_peers, d_res, d_out)
        torch.cuda.synchronize()
        assert d_out.cpu().numpy().tobytes() == want.tobytes(), s
        got = d_res.cpu().numpy()
        assert got.tobytes() == res.tobytes(), s
        assert got[:CHUNK + 1000].any()
        assert not got[CHUNK + 1000:].any()  # the short chunk's tail and the padding slot
        assert not want[2 * SLOT:].any()


# ---- the engine and the drop-in surface ------------------------------------------------------
SGD = dict(lr=0.7, momentum=0.9, nesterov=True)


def test_outer_sync_one_replica_with_error_feedback():
    """OuterSync(world_size=1, int8 wire, error_feedback=True), four steps: the encoder's
    residual and the plain in-place reduce; θ and the momentum against the restatement."""
    rng = np.random.default_rng(83)
    theta, _ = _pseudo_gradient_tree(rng)
    params = [torch.from_numpy(t.copy()).to(DEV) for t in theta]
    eng = OuterSync(params, world_size=1, wire_dtype=torch.int8, error_feedback=True,
                    bucket_cap_elems=CAP, **SGD)
    assert eng.q_residual is not None and eng.q_residual_red is None
    counts = [c1 - c0 for c0, c1 in eng.tree.bucket_chunks]
    ex = ef.EFExchange(NUMELS, counts, 1, reduce_ef=False)
    buf = [np.empty_like(t) for t in theta]
    for s in range(1, 5):
        inner = []
        for t, p in zip(theta, params):
            d = (1e-3 * rng.standard_normal(t.size)).astype(F)
            d[::1500] = 1.0
            inner.append((t - d).astype(F))
            p.copy_(torch.from_numpy(inner[-1]))
        eng.step()
        torch.cuda.synchronize()
        avg = ex.average([[oracle.delta(t, i) for t, i in zip(theta, inner)]])
        for t in range(len(theta)):
            oracle.sgd(theta[t], buf[t], avg[t], SGD["lr"], SGD["momentum"], True, s == 1)
        for t, (g, b, p) in enumerate(zip(eng.unpacked(eng.theta), eng.unpacked(eng.mom), params)):
            assert g.cpu().numpy().tobytes() == theta[t].tobytes(), ("theta", s, t)
            assert b.cpu().numpy().tobytes() == buf[t].tobytes(), ("momentum", s, t)
            assert p.cpu().numpy().tobytes() == theta[t].tobytes(), ("inner", s, t)
    got = eng.unpacked(eng.q_residual)
    for t in range(len(theta)):
        assert got[t].cpu().numpy().tobytes() == ex.enc[0][t].tobytes(), ("residual", t)
    assert bool(eng.q_residual.any())
    eng.close()


class _Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


STEPS = 3


def _flat(ts):
    return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in ts])


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out):
    for p in (PKG, REPO, os.path.join(REPO, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import expect

    os.environ["DILOCO_DP_BACKEND"] = "gloo"
    os.environ["DILOCO_OUTER_BUCKET_ELEMS"] = str(expect.MICRO_Q8_CAP)
    for v in ("DILOCO_OUTER_EXCHANGE", "DILOCO_DP_EXCHANGE", "DILOCO_OUTER_WIRE",
              "DILOCO_OUTER_FUSED", "DILOCO_OUTER_Q8_EF"):
        os.environ.pop(v, None)
    os.environ["DILOCO_COLLECTIVE_READ_TIMEOUT"] = "10"
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank,
                            world_size=world)
    from diloco_amd.comm import TrainingComm
    from diloco_amd.utils import (compute_pseudo_gradient, get_optimizer, get_outer_model,
                                  outer_mirror, q8_error_feedback_state, sync_inner_model)
    from diloco_amd.world import World

    launches = []
    names = ("delta_q8_ef", "q8_reduce_ef", "delta_q8", "q8_reduce")
    for name in names:
        def spy(*a, _f=getattr(K, name), _n=name):
            launches.append(_n)
            return _f(*a)
        setattr(K, name, spy)
    set_default_kernels(K)
    try:
        spec = get_tree("micro")
        numels = spec.numels()
        shapes = [s for _, s in spec.params()]
        theta = synth.outer_tree(numels, spec.init_spec())
        buf = [np.empty_like(t) for t in theta]
        inner = torch.nn.Module()
        inner.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(v.copy()).view(s))
                                           for v, s in zip(theta, shapes)])
        outer = get_outer_model(inner, placement="device", wire="int8", error_feedback=True)
        inner = inner.to(DEV)
        opt = get_optimizer(outer, _Cfg(type="SGD", **SGD))
        comm = TrainingComm(World.from_default_group(1), (1, 1, 32), None)
        rec, ex = {}, None
        for s in range(1, STEPS + 1):
            vals = [synth.inner_tree(theta, s, r) for r in range(world)]
            with torch.no_grad():
                for p, v in zip(inner.parameters(), vals[rank]):
                    p.copy_(torch.from_numpy(v).view(p.shape))
            compute_pseudo_gradient(inner, outer)
            comm.sync_gradients(outer)
            opt.step()
            sync_inner_model(outer, inner)
            if ex is None:
                m = outer_mirror(outer)
                tree = getattr(m, "dev", m).tree
                counts = [c1 - c0 for c0, c1 in tree.bucket_chunks]
                rec["n_buckets"] = np.int64(tree.n_buckets)
                ex = ef.EFExchange(numels, counts, world)
            deltas = [[oracle.delta(t, i) for t, i in zip(theta, v)] for v in vals]
            avg = ex.average(deltas)
            for t in range(len(theta)):
                oracle.sgd(theta[t], buf[t], avg[t], SGD["lr"], SGD["momentum"], True, s == 1)
            torch.cuda.synchronize()
            rec[f"theta_s{s}"] = _flat(outer.parameters())
            rec[f"inner_s{s}"] = _flat(inner.parameters())
            rec[f"ref_theta_s{s}"] = np.concatenate(theta)
        st = q8_error_feedback_state(outer)
        rec["encode_nonzero"] = np.array(bool(st["encode"].any()))
        rec["reduce"] = np.concatenate([a.cpu().numpy() for a in st["reduce"]])
        rec["ref_reduce"] = np.concatenate([ex.red[b][rank] for b in range(len(ex.red))])
        rec["launches"] = np.array(launches)
        np.savez(os.path.join(out, f"r{rank}.npz"), **rec)
    finally:
        set_default_kernels(None)
        for name in names:
            delattr(K, name)
    dist.barrier()
    dist.destroy_process_group()


def test_dropin_int8_wire_error_feedback_two_peers_on_gpu():
    """Two gloo processes on the one GPU, placement="device", error_feedback=True, Nesterov SGD,
    three outer steps: dl_delta_q8_ef -> all_to_all -> dl_q8_reduce_ef -> all_gather ->
    dl_unpack_sgd_q8 per bucket. Both residuals stay local, the averaged slots are the same
    bytes on both ranks, so θ is identical on both and equal to the restatement."""
    out = tempfile.mkdtemp(prefix="dl_q8_ef_")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    recs = [dict(np.load(os.path.join(out, f"r{r}.npz"))) for r in range(2)]
    for rec in recs:
        nb = int(rec["n_buckets"])
        assert nb >= 3
        launches = [str(x) for x in rec["launches"]]
        assert launches.count("delta_q8_ef") == nb * STEPS
        assert launches.count("q8_reduce_ef") == nb * STEPS
        assert "delta_q8" not in launches and "q8_reduce" not in launches
        for s in range(1, STEPS + 1):
            got, want = rec[f"theta_s{s}"], rec[f"ref_theta_s{s}"]
            assert got.tobytes() == want.tobytes(), (s, int((got != want).sum()))
            assert rec[f"inner_s{s}"].tobytes() == want.tobytes(), s
            assert got.tobytes() == recs[0][f"theta_s{s}"].tobytes(), s
        assert bool(rec["encode_nonzero"])
        assert rec["reduce"].tobytes() == rec["ref_reduce"].tobytes()
