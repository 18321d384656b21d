"""The rotated fp4 wire on the GPU against the numpy restatement (tests/fp4_rot_restatement.py over
tests/fp4_restatement.py), bit for bit, NaNs by position. The tree: one element, one short of and
one past a 256-element block, a one-element spill into a second chunk, a three-chunk tensor whose
tail is no multiple of 4; bucket cap 8192 splits it. Padding holds a NaN sentinel, slots 0xEE."""
import functools
import os
import socket
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import fp4_restatement as fp4
import fp4_rot_restatement as rot
from conftest import PKG, REPO
from diloco_amd import _lib
from diloco_amd.kernels import HipKernels, adamw_scalars
from diloco_amd.plan import SLOT_INNER, PackedTree
from oracle_kernels import CpuTree

pytestmark = pytest.mark.gpu
DEV, F = "cuda:0", np.float32
NUMELS, CAP = [1, 255, 257, 4097, 8217], 8192
SLOT, CHUNK, ALL = fp4.SLOT, fp4.CHUNK, _lib.ALL_BUCKETS
SEED = 0x5EED
LR, MOMENTUM = 0.7, 0.9
ADAM = adamw_scalars(0.01, 0.9, 0.95, 0.1, 1e-8, 2)
K = HipKernels()


def _sentinels(n):
    return np.full(n, 0x7F8BEEF5, dtype=np.uint32).view(F)  # a NaN bit pattern


@functools.lru_cache(maxsize=None)
def _case(ef, wild=False):
    """(θ, inner, residual) per tensor and the restatement's (slots, residual, decoded wire) in
    the packed layout, sentinel padding included."""
    rng = np.random.default_rng(5)
    theta = [rng.standard_normal(n).astype(F) for n in NUMELS]
    inner = [(t - (0.01 * rng.standard_t(3, t.size)).astype(F)).astype(F) for t in theta]
    resid = [(1e-3 * rng.standard_normal(n) * ef).astype(F) for n in NUMELS]
    if wild:  # the first two blocks of the three-chunk tensor's second chunk
        inner[4][4096 + 10], theta[4][4096 + 300] = np.nan, np.inf
    cpu = CpuTree(NUMELS, CAP)
    slots = np.empty(len(cpu.chunks) * SLOT, dtype=np.uint8)
    res, wire = _sentinels(cpu.total), _sentinels(cpu.total)
    for c, (seg, o, n, po) in enumerate(cpu.chunks):
        r = resid[seg][o:o + n]
        s, r2 = rot.encode_chunk(theta[seg][o:o + n], inner[seg][o:o + n], SEED, r if ef else None)
        slots[c * SLOT:(c + 1) * SLOT] = s
        res[po:po + n] = r2 if ef else r  # the plain encoder never touches a residual
        wire[po:po + n] = rot.decode_chunk(s, SEED, n)
    return theta, inner, resid, slots, res, wire


class _Rig:
    """The tree on the device; inner tensors 16-B aligned or one float off."""

    def __init__(self, theta, inner, resid, misaligned=False):
        self.tree = PackedTree(NUMELS, CAP)
        assert self.tree.n_buckets >= 2
        self.offs = [int(o) for o in self.tree.seg_off[:-1]]
        self.pad = np.ones(self.tree.total, dtype=bool)
        th, rs = _sentinels(self.tree.total), _sentinels(self.tree.total)
        for i, (o, n) in enumerate(zip(self.offs, NUMELS)):
            self.pad[o:o + n], th[o:o + n], rs[o:o + n] = False, theta[i], resid[i]
        self.theta, self.resid = torch.from_numpy(th).to(DEV), torch.from_numpy(rs).to(DEV)
        self.slots = torch.full((self.tree.n_chunks * SLOT,), 0xEE, dtype=torch.uint8, device=DEV)
        base = torch.zeros(sum(NUMELS) + 8 * len(NUMELS) + 8, dtype=torch.float32, device=DEV)
        self.inner, at = [], int(misaligned)
        for n, v in zip(NUMELS, inner):
            self.inner.append(base[at:at + n].copy_(torch.from_numpy(v)))
            assert self.inner[-1].data_ptr() % 16 == 4 * misaligned
            at += n + (-n) % 4 + 4
        self.tree.bind(SLOT_INNER, self.inner, torch.cuda.current_stream().cuda_stream)

    def launch(self, whole, f):
        """f(bucket, that bucket's slots): one whole-tree launch or bucket by bucket."""
        for b, (c0, c1) in enumerate([(0, self.tree.n_chunks)] if whole else self.tree.bucket_chunks):
            f(ALL if whole else b, self.slots[c0 * SLOT:c1 * SLOT])

    def packed(self, rng, square=False):
        x = _sentinels(self.tree.total)
        v = rng.standard_normal(int((~self.pad).sum())).astype(F)
        x[~self.pad] = v * v * F(0.01) if square else v
        return torch.from_numpy(x).to(DEV)


def _same(got, want, pad, what):
    """Bit for bit inside, NaNs by position; the padding still holds the sentinel."""
    got, want = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in (got, want))
    assert fp4.same_bits(got[~pad], want[~pad]), what
    assert got[pad].tobytes() == _sentinels(int(pad.sum())).tobytes(), (what, "padding")


@pytest.mark.parametrize("whole", [False, True])
@pytest.mark.parametrize("ef", [False, True])
@pytest.mark.parametrize("misaligned", [False, True])
def test_rot_kernels_match_the_restatement(misaligned, ef, whole):
    theta, inner, resid, want_slots, want_res, want_wire = _case(ef)
    a, b = (_Rig(theta, inner, resid, misaligned) for _ in range(2))  # b: the fp32-wire twin
    a.launch(whole, lambda k, s: K.delta_fp4_rot(a.tree, k, SLOT_INNER, a.theta,
                                                 a.resid if ef else None, SEED, s))
    assert a.slots.cpu().numpy().tobytes() == want_slots.tobytes()
    _same(a.resid, want_res, a.pad, "residual")
    dst = torch.from_numpy(_sentinels(a.tree.total)).to(DEV)
    a.launch(whole, lambda k, s: K.decode_fp4_rot(a.tree, k, s, SEED, dst))
    _same(dst, want_wire, a.pad, "decode")
    # the fused steps against dl_unpack_sgd / dl_unpack_adamw on the restatement's decoded wire
    wire, rng = torch.from_numpy(want_wire).to(DEV), np.random.default_rng(9)
    st = [a.packed(rng), a.packed(rng), a.packed(rng, square=True)]
    mom, m1, m2 = st
    mom_b, m1_b, m2_b = (x.clone() for x in st)
    a.launch(whole, lambda k, s: K.unpack_sgd_fp4_rot(a.tree, k, s, SEED, a.theta, mom, LR,
                                                      MOMENTUM, True, False, SLOT_INNER))
    a.launch(whole, lambda k, s: K.unpack_adamw_fp4_rot(a.tree, k, s, SEED, a.theta, m1, m2,
                                                        ADAM, SLOT_INNER))
    K.unpack_sgd(b.tree, ALL, wire, 1, b.theta, mom_b, LR, MOMENTUM, True, False, SLOT_INNER)
    K.unpack_adamw(b.tree, ALL, wire, 1, b.theta, m1_b, m2_b, ADAM, SLOT_INNER)
    for x, y, what in [(a.theta, b.theta, "theta"), (mom, mom_b, "momentum"),
                       (m1, m1_b, "exp_avg"), (m2, m2_b, "exp_avg_sq")]:
        _same(x, y, a.pad, what)
    for i, (x, y) in enumerate(zip(a.inner, b.inner)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), ("inner", i)
    a.tree.close()
    b.tree.close()


def test_a_non_finite_value_takes_its_block_and_no_other():
    theta, inner, resid, want_slots, _res, want_wire = _case(False, True)
    rig = _Rig(theta, inner, resid)
    K.delta_fp4_rot(rig.tree, ALL, SLOT_INNER, rig.theta, None, SEED, rig.slots)
    dst = torch.from_numpy(_sentinels(rig.tree.total)).to(DEV)
    K.decode_fp4_rot(rig.tree, ALL, rig.slots, SEED, dst)
    assert rig.slots.cpu().numpy().tobytes() == want_slots.tobytes()
    _same(dst, want_wire, rig.pad, "decode")
    got, at = dst.cpu().numpy()[~rig.pad], sum(NUMELS[:4]) + 4096
    assert np.isnan(got[at:at + 512]).all() and np.isnan(got).sum() == 512
    rig.tree.close()


def test_rotation_lowers_the_error_on_a_heavy_tail():
    """One full chunk of Student-t(3): the restatement alone gives 0.119 rotated against 0.152."""
    x = np.random.default_rng(0).standard_t(3, CHUNK).astype(F)
    tree = PackedTree([CHUNK], CAP)
    inner = [torch.zeros(CHUNK, device=DEV)]  # bound by address: kept alive to the end
    tree.bind(SLOT_INNER, inner, torch.cuda.current_stream().cuda_stream)
    theta, dst = torch.from_numpy(x).to(DEV), torch.zeros(CHUNK, device=DEV)
    plain, turned = (torch.zeros(SLOT, dtype=torch.uint8, device=DEV) for _ in range(2))
    K.delta_fp4(tree, ALL, SLOT_INNER, theta, None, plain)
    K.delta_fp4_rot(tree, ALL, SLOT_INNER, theta, None, SEED, turned)
    K.decode_fp4_rot(tree, ALL, turned, SEED, dst)
    e_plain, e_rot = (np.linalg.norm(y.astype(np.float64) - x) / np.linalg.norm(x.astype(np.float64))
                      for y in (fp4.decode_slot(plain.cpu().numpy()), dst.cpu().numpy()))
    print(f"relative L2 error: plain {e_plain:.4f}, rotated {e_rot:.4f}")
    assert e_rot < e_plain
    tree.close()


def _worker(rank, port):
    for p in (PKG, REPO, os.path.join(REPO, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(DILOCO_OUTER_BUCKET_ELEMS=str(CAP), DILOCO_OUTER_FP4_SEED="0x1234")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    from diloco_amd.utils import (compute_pseudo_gradient, get_optimizer, get_outer_model,
                                  outer_mirror, sync_inner_model)

    rng = np.random.default_rng(3)
    inner = torch.nn.Module()
    inner.ps = torch.nn.ParameterList(
        [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(n).astype(F))) for n in NUMELS])
    inner = inner.to(DEV)
    outer = get_outer_model(inner, placement="device", wire="fp4", rotate=True, error_feedback=True)
    opt = get_optimizer(outer, SimpleNamespace(type="SGD", lr=LR, momentum=MOMENTUM, nesterov=True))
    m, ps, ins = outer_mirror(outer), list(outer.parameters()), list(inner.parameters())
    assert m.rotate and m.rot_seed == 0x1234 and m.tree.n_buckets >= 2
    tree = PackedTree(NUMELS, CAP)  # the twin: its own arenas, whole-tree launches
    offs = [int(o) for o in tree.seg_off[:-1]]
    theta, mom, res, wire = (torch.zeros(tree.total, device=DEV) for _ in range(4))
    res2 = torch.zeros(tree.n_chunks * CHUNK, device=DEV)
    slots = torch.zeros(tree.n_chunks * SLOT, dtype=torch.uint8, device=DEV)
    for o, p in zip(offs, ps):
        theta[o:o + p.numel()] = p.detach()
    for s in (1, 2):
        with torch.no_grad():
            for p in ins:
                p.add_(torch.from_numpy((0.01 * rng.standard_t(3, p.numel())).astype(F)).to(DEV))
        twin = [p.detach().clone() for p in ins]
        compute_pseudo_gradient(inner, outer)
        m.all_reduce(dist.group.WORLD, 1)
        opt.step()
        sync_inner_model(outer, inner)
        tree.bind(SLOT_INNER, twin, torch.cuda.current_stream().cuda_stream)
        K.delta_fp4_rot(tree, ALL, SLOT_INNER, theta, res, 0x1234, slots)
        K.fp4_reduce(slots, 1, tree.n_chunks, 1, res2, slots)
        K.unpack_sgd_fp4_rot(tree, ALL, slots, 0x1234, theta, mom, LR, MOMENTUM, True, s == 1,
                             SLOT_INNER)
        K.decode_fp4_rot(tree, ALL, slots, 0x1234, wire)
        for i, (o, n) in enumerate(zip(offs, NUMELS)):
            for x, y in [(ps[i].detach(), theta), (opt.state[ps[i]]["momentum_buffer"], mom),
                         (ps[i].grad, wire)]:
                assert torch.equal(x.view(torch.int32), y[o:o + n].view(torch.int32)), (s, i)
            assert torch.equal(ins[i].detach().view(torch.int32), twin[i].view(torch.int32))
        assert wire.any() and res.any()
    tree.close()
    dist.destroy_process_group()


def test_dropin_rotated_fp4_wire_at_one_replica():
    """get_outer_model(wire="fp4", rotate=True, error_feedback=True) through the reference's calls
    for two outer steps, in a process of its own with a one-rank gloo group. At one replica
    sync_gradients returns at once, so the exchange it makes at N > 1 (the mirror's all_reduce) is
    called directly. θ, the momentum, inner and the .grad read equal the same launches made by
    hand on a twin, bit for bit (asserted in the worker; a failing worker fails the spawn)."""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mp.spawn(_worker, args=(port,), nprocs=1, join=True)
