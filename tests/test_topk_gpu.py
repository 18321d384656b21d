"""The top-k sparse wire on the GPU: dl_delta_topk, dl_topk_reduce, dl_unpack_sgd_topk and
dl_unpack_adamw_topk against the numpy restatement (tests/topk_restatement.py), bit for bit, NaNs
by position; nothing is skipped or masked. The tree is test_fp4_gpu.py's: several buckets, a
chunk shorter than k, one short of full, spills of 1 and 3 elements, tails no multiple of 4;
inner tensors 16-B aligned or one float off; slots pre-filled with 0xEE; the packed arenas'
padding holds a NaN sentinel that must survive."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import topk_restatement as tk
from conftest import PKG, REPO
from diloco_amd import _lib, synth
from diloco_amd.kernels import HipKernels, adamw_scalars
from diloco_amd.mirror import _decode_topk
from diloco_amd.plan import SLOT_INNER, PackedTree
from diloco_amd.trees import get_tree
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV, F, ALL = "cuda:0", np.float32, _lib.ALL_BUCKETS
NUMELS = [1, 31, 33, 4095, 4096, 4097, 4099, 8217, 14338]
SENTINEL = 0x7F8BEEF5
K = HipKernels()


def _same_slots(got, want, k, what):
    got, want = got.cpu().numpy().reshape(-1, 6 * k), want.reshape(-1, 6 * k)
    assert got[:, 4 * k:].tobytes() == want[:, 4 * k:].tobytes(), (what, "indices")
    assert tk.same_bits(got[:, :4 * k].copy().view(F), want[:, :4 * k].copy().view(F)), what


class _Rig:
    """One tree on the device: packed arenas whose padding holds the sentinel, inner tensors."""

    def __init__(self, k, misaligned, numels=NUMELS):
        self.k, self.numels = k, numels
        self.tree = PackedTree(numels, 8192)
        self.offs = [int(o) for o in self.tree.seg_off[:-1]]
        self.pad = np.ones(self.tree.total, dtype=bool)
        for o, n in zip(self.offs, numels):
            self.pad[o:o + n] = False
        self.slots = torch.zeros(self.tree.n_chunks * 6 * k, dtype=torch.uint8, device=DEV)
        base = torch.zeros(sum(numels) + 8 * len(numels) + 8, device=DEV)
        self.inner, at = [], int(misaligned)
        for n in numels:
            self.inner.append(base[at:at + n])
            assert self.inner[-1].data_ptr() % 16 == 4 * int(misaligned)
            at += n + (-n) % 4 + 4
        self.tree.bind(SLOT_INNER, self.inner, torch.cuda.current_stream().cuda_stream)

    def packed(self, tensors):
        a = np.full(self.tree.total, SENTINEL, dtype=np.uint32).view(F)
        for o, t in zip(self.offs, tensors):
            a[o:o + t.size] = t
        return torch.from_numpy(a).to(DEV)

    def check(self, got, want, what):
        got = got.cpu().numpy()
        assert (got.view(np.uint32)[self.pad] == SENTINEL).all(), (what, "padding")
        assert tk.same_bits(got[~self.pad], np.concatenate(want)), what

    def encode(self, theta, inner, resid, mode="buckets"):
        for d, i in zip(self.inner, inner):
            d.copy_(torch.from_numpy(i))
        th = self.packed(theta)
        res = self.packed(resid) if resid is not None else None
        self.slots.fill_(0xEE)
        self.tree.tune(3 if mode == "grid3" else 0)
        S = 6 * self.k
        for b in ([ALL] if mode != "buckets" else range(self.tree.n_buckets)):
            c0 = 0 if b == ALL else self.tree.bucket_chunks[b][0]
            K.delta_topk(self.tree, b, SLOT_INNER, th, res, self.k, self.slots[c0 * S:])
        torch.cuda.synchronize()
        return res


def _expect(theta, inner, resid, k):
    enc = [tk.encode_tensor(t - i, k, r) for t, i, r in
           zip(theta, inner, resid if resid is not None else [None] * len(theta))]
    return np.concatenate([s for s, _ in enc]), [r for _, r in enc]


def _decades(rng, n):  # magnitudes spread over five decades
    return (10.0 ** rng.uniform(-5, 0, n) * rng.choice([-1.0, 1.0], n)).astype(F)


@pytest.mark.parametrize("k", [8, 64, 256])
@pytest.mark.parametrize("ef", [False, True])
@pytest.mark.parametrize("misaligned", [False, True])
def test_delta_topk_matches_the_restatement(misaligned, ef, k):
    rng = np.random.default_rng(k)
    rig = _Rig(k, misaligned)
    theta = [rng.standard_normal(n).astype(F) for n in NUMELS]
    inner = [(t - _decades(rng, t.size)).astype(F) for t in theta]
    resid = [_decades(rng, n) for n in NUMELS] if ef else None
    want_s, want_r = _expect(theta, inner, resid, k)
    for mode in ("buckets", "whole", "grid3"):
        res = rig.encode(theta, inner, resid, mode)
        _same_slots(rig.slots, want_s, k, mode)
        if ef:
            rig.check(res, want_r, (mode, "residual"))
    rig.tree.close()


N = tk.CHUNK


def _put(idx, vals, base=0.0):
    x = np.full(N, base, dtype=F)
    x[idx] = vals
    return x


def _u32(a):
    return np.asarray(a).astype(np.uint32).view(F)


EDGE = {  # name -> (rng, k) -> one chunk
    "pm1": lambda r, k: r.choice([-1.0, 1.0], N).astype(F),  # the k lowest indices win
    # k - 1 large values over a plateau from index 3 on: exactly one tie is taken, the lowest
    "plateau": lambda r, k: _put(np.r_[:3, r.choice(np.arange(3, N), k - 1, replace=False)],
                                 [0.25] * 3 + [2.0] * (k - 1), 0.5),
    "low7": lambda r, k: _u32(0x3F800000 | r.integers(0, 128, N)),
    "midbyte": lambda r, k: _u32(0x3F800000 | (r.integers(0, 256, N) << 11)),
    "denormals": lambda r, k: _put(r.choice(N, 240, replace=False),  # and -0 among the zeros
                                   np.r_[_u32(r.integers(1, 1 << 22, 40)), [-0.0] * 200]),
    "few": lambda r, k: _put(r.choice(N, k // 2, replace=False), 1.5),
    "nan_inf": lambda r, k: _put([77, 3001], [np.nan, -np.inf], r.standard_normal(N)),
    "many_inf": lambda r, k: _put(r.choice(N, k + 9, replace=False),  # more than k non-finite
                                  r.choice([np.inf, -np.inf], k + 9), r.standard_normal(N)),
}


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("name", list(EDGE))
def test_selection_edge_cases(name, misaligned):
    k, rng = 64, np.random.default_rng(5)
    rig = _Rig(k, misaligned, [tk.CHUNK])
    theta, inner = [EDGE[name](rng, k)], [np.zeros(N, dtype=F)]  # x - (+0) = x bit for bit
    resid = [np.zeros(tk.CHUNK, dtype=F)]
    with np.errstate(all="ignore"):
        want_s, want_r = _expect(theta, inner, resid, k)
    idx = want_s[4 * k:].view(np.uint16)
    assert name != "pm1" or idx.tolist() == list(range(k))
    assert name != "plateau" or ((theta[0][idx] == 2.0).sum() == k - 1 and idx[0] == 3)
    res = rig.encode(theta, inner, resid, "whole")
    _same_slots(rig.slots, want_s, k, name)
    rig.check(res, want_r, (name, "residual"))
    rig.encode(theta, inner, None, "whole")  # no residual add: -0 reaches the slot as it is
    _same_slots(rig.slots, _expect(theta, inner, None, k)[0], k, (name, "plain"))
    rig.tree.close()


@pytest.mark.parametrize("ef", [False, True])
@pytest.mark.parametrize("n,divisor", [(1, 1), (2, 2), (3, 3), (3, 1)])
def test_topk_reduce_matches_the_restatement(n, divisor, ef):
    k, m, rng = 64, 3, np.random.default_rng(10 * n + divisor)
    shared = rng.choice(tk.CHUNK, 40, replace=False)  # overlapping and disjoint indices
    slots = []
    for r in range(n):
        for j in range(m):
            x = (_decades(rng, tk.CHUNK) * F(1e-3)).astype(F)
            x[shared] = rng.standard_normal(40).astype(F)
            x[rng.choice(tk.CHUNK, 30, replace=False)] = rng.standard_normal(30).astype(F)
            slots.append(tk.select(x, k, False)[0] if (r, j) != (0, 1) else np.zeros(6 * k, np.uint8))
    recv = np.concatenate(slots)
    res0 = _decades(rng, m * tk.CHUNK) if ef else None
    want, want_r = tk.reduce_slots(recv, n, m, divisor, k, res0)
    d_recv = torch.from_numpy(recv).to(DEV)
    out = d_recv if n == 1 else torch.full((m * 6 * k,), 0xEE, dtype=torch.uint8, device=DEV)
    res = torch.from_numpy(res0).to(DEV) if ef else None
    K.topk_reduce(d_recv, n, m, divisor, res, k, out)
    _same_slots(out, want, k, (n, divisor, ef))
    if ef:
        assert tk.same_bits(res.cpu().numpy(), want_r)


ADAM = adamw_scalars(0.01, 0.9, 0.95, 0.1, 1e-8, 2)


@pytest.mark.parametrize("write_inner", [True, False])
@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("rule", ["sgd0", "nesterov", "adamw"])
def test_unpack_topk_equals_decode_then_unpack(rule, misaligned, write_inner):
    k, rng = 64, np.random.default_rng(23)
    rigs = [_Rig(k, misaligned), _Rig(k, misaligned)]  # the fused pass; decode + the fp32 pass
    slots, _ = _expect([_decades(rng, n) for n in NUMELS], [np.zeros(n, dtype=F) for n in NUMELS],
                       None, k)
    dense = _decode_topk(torch.from_numpy(slots).to(DEV).view(-1, 6 * k), k).cpu().numpy()
    wire, c = [], 0
    for n in NUMELS:
        nch = -(-n // tk.CHUNK)
        wire.append(dense[c:c + nch].reshape(-1)[:n])
        c += nch
    theta0 = [rng.standard_normal(n).astype(F) for n in NUMELS]
    state0 = [[np.abs(rng.standard_normal(n)).astype(F) for n in NUMELS] for _ in range(2)]
    inner0 = [rng.standard_normal(n).astype(F) for n in NUMELS]
    slot = SLOT_INNER if write_inner else -1
    outs = []
    for fused, rig in zip((True, False), rigs):
        for d, i in zip(rig.inner, inner0):
            d.copy_(torch.from_numpy(i))
        th, m1, m2 = rig.packed(theta0), rig.packed(state0[0]), rig.packed(state0[1])
        src = torch.from_numpy(slots).to(DEV) if fused else rig.packed(wire)
        hp = (0.7, 0.0, False, False) if rule == "sgd0" else (0.7, 0.9, True, False)
        if rule == "adamw":
            (K.unpack_adamw_topk(rig.tree, ALL, src, k, th, m1, m2, ADAM, slot) if fused else
             K.unpack_adamw(rig.tree, ALL, src, 1, th, m1, m2, ADAM, slot))
        else:
            (K.unpack_sgd_topk(rig.tree, ALL, src, k, th, m1, *hp, slot) if fused else
             K.unpack_sgd(rig.tree, ALL, src, 1, th, m1, *hp, slot))
        torch.cuda.synchronize()
        outs.append([a.cpu().numpy() for a in (th, m1, m2, *rig.inner)])
    for a, b in zip(*outs):  # padding sentinels included: whole arenas, byte for byte
        assert a.tobytes() == b.tobytes()
    assert (outs[0][0].view(np.uint32)[rigs[0].pad] == SENTINEL).all()
    assert not write_inner or tk.same_bits(np.concatenate(outs[0][3:]), outs[0][0][~rigs[0].pad])
    for rig in rigs:
        rig.tree.close()


SGD = dict(lr=0.7, momentum=0.9, nesterov=True)
ADAMW = dict(lr=0.01, betas=(0.9, 0.95), weight_decay=0.1)


def _worker(rank, world, port, rule):
    for p in (PKG, REPO, os.path.join(REPO, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import expect
    from types import SimpleNamespace

    os.environ.update(DILOCO_DP_BACKEND="gloo", DILOCO_OUTER_ADAMW="fused",
                      DILOCO_OUTER_BUCKET_ELEMS=str(expect.MICRO_Q8_CAP),
                      DILOCO_COLLECTIVE_READ_TIMEOUT="10")
    for v in ("DILOCO_OUTER_EXCHANGE", "DILOCO_DP_EXCHANGE", "DILOCO_OUTER_WIRE",
              "DILOCO_OUTER_FUSED", "DILOCO_OUTER_TOPK", "DILOCO_OUTER_TOPK_EF"):
        os.environ.pop(v, None)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank,
                            world_size=world)
    from adamw_restatement import AdamWState
    from diloco_amd.comm import TrainingComm
    from diloco_amd.utils import (compute_pseudo_gradient, get_optimizer, get_outer_model,
                                  outer_mirror, q8_error_feedback_state, sync_inner_model)
    from diloco_amd.world import World

    spec = get_tree("micro")
    numels, shapes = spec.numels(), [s for _, s in spec.params()]
    theta0 = synth.outer_tree(numels, spec.init_spec())
    inner = torch.nn.Module()
    inner.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(v.copy()).view(s))
                                       for v, s in zip(theta0, shapes)])
    outer = get_outer_model(inner, placement="device", wire="topk", topk=64)  # EF: on by default
    inner = inner.to(DEV)
    opt = get_optimizer(outer, SimpleNamespace(type="SGD" if rule == "sgd" else "AdamW",
                                               **(SGD if rule == "sgd" else ADAMW)))
    ref = AdamWState(theta0, **ADAMW)
    theta, buf = [t.copy() for t in theta0], [np.empty_like(t) for t in theta0]
    comm = TrainingComm(World.from_default_group(1), (1, 1, 32), None)
    ex = None

    def flat(ts):
        return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in ts])
    for s in (1, 2, 3):
        vals = [synth.inner_tree(theta, s, r) for r in range(world)]
        with torch.no_grad():
            for p, v in zip(inner.parameters(), vals[rank]):
                p.copy_(torch.from_numpy(v).view(p.shape))
        compute_pseudo_gradient(inner, outer)
        comm.sync_gradients(outer)
        opt.step()
        sync_inner_model(outer, inner)
        if ex is None:  # the mirror exists once the first pseudo-gradient named the device
            dev = getattr(outer_mirror(outer), "dev", outer_mirror(outer))
            assert dev.tree.n_buckets >= 3
            ex = tk.TopkExchange(numels, [c1 - c0 for c0, c1 in dev.tree.bucket_chunks], world, 64)
        avg = ex.average([[oracle.delta(t, i) for t, i in zip(theta, v)] for v in vals])
        if rule == "sgd":
            for t in range(len(theta)):
                oracle.sgd(theta[t], buf[t], avg[t], SGD["lr"], SGD["momentum"], True, s == 1)
        else:
            ref.step_grads(avg)
            theta = ref.theta
        torch.cuda.synchronize()
        # byte for byte the restatement's θ on every rank, so byte-identical across ranks
        assert flat(outer.parameters()).tobytes() == np.concatenate(theta).tobytes(), s
        assert flat(inner.parameters()).tobytes() == np.concatenate(theta).tobytes(), s
        assert tk.same_bits(flat([p.grad for p in outer.parameters()]), np.concatenate(avg)), s
    st = q8_error_feedback_state(outer)
    enc = st["encode"].cpu().numpy()
    enc = np.concatenate([enc[o:o + n] for o, n in zip(dev.offs, numels)])
    red = np.concatenate([a.cpu().numpy() for a in st["reduce"]])
    assert tk.same_bits(enc, np.concatenate(ex.enc[rank])) and enc.any()
    assert tk.same_bits(red, np.concatenate([r[rank] for r in ex.red])) and red.any()
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("rule", ["sgd", "adamw"])
def test_dropin_topk_wire_two_peers_on_gpu(rule):
    """Two gloo processes on the one GPU, placement="device", wire="topk", topk=64, three outer
    steps: θ, inner, .grad and both residuals equal the restatement's exchange on both ranks
    (asserted inside each rank; a failing rank fails the spawn)."""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mp.spawn(_worker, args=(2, port, rule), nprocs=2, join=True)
