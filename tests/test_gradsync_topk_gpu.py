"""The top-k wire of the per-step DP gradient sync on the GPU: dl_gather_topk[_fp4] and
dl_unpack_avg_topk[_fp4] against the numpy restatements (tests/topk_restatement.py,
tests/topk_fp4_restatement.py, tests/clip_restatement.py), GradSync and TrainingComm on top of
them against the restated exchange. Bit for bit, NaNs by position; nothing is skipped or masked.

The tree is tests/gradsync_fp4_inputs.py's (chunks shorter than k, tails no multiple of 4, a chunk
one short of full, a one-element spill; several buckets). Gradients are views into one
sentinel-filled buffer with guard floats between them, 16-B aligned or one float off; slots start
as 0xFF between two guard slots, the residual arena's padding as a NaN bit pattern."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import clip_restatement as cr
import topk_fp4_restatement as tq
import topk_restatement as tk
from conftest import PKG, REPO
from diloco_amd import _lib, utils
from diloco_amd.gradsync import GradSync, slot_wire_bytes
from diloco_amd.kernels import HipKernels
from diloco_amd.plan import SLOT_GRAD, SLOT_INNER, PackedTree
from gradsync_fp4_inputs import CAP, NUMELS, groupwise, special

pytestmark = pytest.mark.gpu
DEV, F, ALL = "cuda:0", np.float32, _lib.ALL_BUCKETS
NAN_BITS, GUARD, SENTINEL, PART_SENTINEL = 0x7F8BEEF5, 4, F(-123.25), -7.0
K = HipKernels()
# values -> (restatement, encoder, decoder, the outer step's encoder)
WIRES = {"f32": (tk, K.gather_topk, K.unpack_avg_topk, K.delta_topk),
         "fp4": (tq, K.gather_topk_fp4, K.unpack_avg_topk_fp4, K.delta_topk_fp4)}
VALUES = pytest.mark.parametrize("values", list(WIRES))
ALIGN = pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])


def tied(seed):
    """groupwise() with 300 elements of every chunk of the two largest tensors at the chunk's
    largest magnitude, signs mixed: more than any k share it, the lowest indices win."""
    out, rng = groupwise(seed), np.random.default_rng(seed)
    for t in out[-2:]:
        for o in range(0, t.size - 300, tk.CHUNK):
            at = o + rng.choice(min(tk.CHUNK, t.size - o), 300, replace=False)
            t[at] = rng.choice([-1.0, 1.0], 300)
    return out


def _decoded(ref, slots, k, numels=NUMELS):
    """The tensors a tree's slots decode to."""
    S = slots.size // sum(-(-n // tk.CHUNK) for n in numels)
    vals, c = [], 0
    for n in numels:
        nch = -(-n // tk.CHUNK)
        vals.append(np.concatenate([ref.decode(slots[j * S:(j + 1) * S], k)
                                    for j in range(c, c + nch)])[:n])
        c += nch
    return vals


# k with the launch (whole tree / bucket by bucket / three workgroups walking the chunks) and input
CASES = [(8, "whole", special), (64, "buckets", tied), (256, "grid3", groupwise)]


class _Rig:
    def __init__(self, k, values, misaligned, mode):
        self.k, self.S, self.mode = k, slot_wire_bytes("topk", k, values), mode
        self.tree = PackedTree(NUMELS, CAP)
        self.tree.tune(3 if mode == "grid3" else 0)
        assert self.tree.n_buckets >= 3
        self.nch = self.tree.n_chunks
        self.offs = [int(o) for o in self.tree.seg_off[:-1]]
        self.pad = np.ones(self.tree.total, dtype=bool)
        self.at, at = [], GUARD + int(misaligned)
        for o, n in zip(self.offs, NUMELS):
            self.pad[o:o + n] = False
            self.at.append(at)
            at += n + GUARD + (-(n + GUARD)) % 4
        self.base = torch.full((at + GUARD,), float(SENTINEL), device=DEV)
        self.grads = [self.base[a:a + n] for a, n in zip(self.at, NUMELS)]
        assert all(g.data_ptr() % 16 == 4 * int(misaligned) for g in self.grads)
        self.guard = np.ones(self.base.numel(), dtype=bool)
        for a, n in zip(self.at, NUMELS):
            self.guard[a:a + n] = False
        self.tree.bind(SLOT_GRAD, self.grads, torch.cuda.current_stream().cuda_stream)
        self.resid = torch.from_numpy(np.where(self.pad, NAN_BITS, 0).astype(np.uint32).view(F)).to(DEV)
        self.all_slots = torch.full(((self.nch + 2) * self.S,), 0xFF, dtype=torch.uint8, device=DEV)
        self.slots = self.all_slots[self.S:-self.S]

    def launch(self, fn):
        """fn(bucket, the bucket's slots) for the whole tree or bucket by bucket, last first."""
        for b in ([ALL] if self.mode != "buckets" else reversed(range(self.tree.n_buckets))):
            fn(b, self.slots[(0 if b == ALL else self.tree.bucket_chunks[b][0]) * self.S:])
        torch.cuda.synchronize()

    def guards_hold(self):
        s = self.all_slots.cpu().numpy()
        assert (s[:self.S] == 0xFF).all() and (s[-self.S:] == 0xFF).all()
        assert (self.base.cpu().numpy()[self.guard] == SENTINEL).all()

    def residual(self):
        r = self.resid.cpu().numpy()
        assert (r.view(np.uint32)[self.pad] == NAN_BITS).all()
        return [r[o:o + n] for o, n in zip(self.offs, NUMELS)]


# ---- 1: the encoder --------------------------------------------------------------------------
@VALUES
@ALIGN
@pytest.mark.parametrize("ef", [False, True], ids=["plain", "ef"])
@pytest.mark.parametrize("k,mode,make", CASES, ids=[f"k{c[0]}-{c[1]}" for c in CASES])
def test_gather_topk_matches_the_restatement(k, mode, make, ef, misaligned, values):
    """Two consecutive steps: the second starts from the residual the first left."""
    ref, gather = WIRES[values][:2]
    rig = _Rig(k, values, misaligned, mode)
    res = [np.zeros(n, dtype=F) for n in NUMELS] if ef else [None] * len(NUMELS)
    for step in (1, 2):
        g = make(10 * k + step)
        for d, x in zip(rig.grads, g):
            d.copy_(torch.from_numpy(x))
        with np.errstate(all="ignore"):
            enc = [ref.encode_tensor(x, k, r) for x, r in zip(g, res)]
        res = [r for _, r in enc]
        rig.all_slots.fill_(0xFF)
        rig.launch(lambda b, s: gather(rig.tree, b, SLOT_GRAD, rig.resid if ef else None, k, s))
        want = np.concatenate([s for s, _ in enc])
        assert rig.slots.cpu().numpy().tobytes() == want.tobytes(), step  # every byte written
        rig.guards_hold()
        got_r = rig.residual()
        if ef:
            assert tk.same_bits(np.concatenate(got_r), np.concatenate(res)), step
            assert np.concatenate(res).any()
        else:
            assert not np.concatenate(got_r).any()
        for d, x in zip(rig.grads, g):  # the gradients are only read
            assert tk.same_bits(d.cpu().numpy(), x)
    rig.tree.close()


@VALUES
def test_gather_topk_equals_delta_topk_with_a_zero_inner(values):
    """outer = g, inner = +0: byte for byte, the residual too."""
    gather, delta = WIRES[values][1], WIRES[values][3]
    rig, g = _Rig(64, values, True, "whole"), special(7)
    theta = torch.zeros(rig.tree.total, device=DEV)
    for o, d, x, r in zip(rig.offs, rig.grads, g, groupwise(8)):
        d.copy_(torch.from_numpy(x))
        theta[o:o + x.size] = d
        rig.resid[o:o + x.size] = torch.from_numpy(r * F(0.01))
    zeros = torch.zeros(rig.base.numel(), device=DEV)
    rig.tree.bind(SLOT_INNER, [zeros[a:a + n] for a, n in zip(rig.at, NUMELS)],
                  torch.cuda.current_stream().cuda_stream)
    r_b, other = rig.resid.clone(), torch.full_like(rig.all_slots, 0xFF)
    gather(rig.tree, ALL, SLOT_GRAD, rig.resid, 64, rig.slots)
    delta(rig.tree, ALL, SLOT_INNER, theta, r_b, 64, other[rig.S:-rig.S])
    torch.cuda.synchronize()
    assert torch.equal(rig.all_slots, other)
    assert torch.equal(rig.resid.view(torch.int32), r_b.view(torch.int32))
    rig.tree.close()


# ---- 2: the decoder --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def averaged():
    """(values, k) -> slots as an exchange leaves them (two peers' encoded slots through the
    restated reduce; a NaN and an Inf among the entries; chunk 3's slot all zero bytes), the
    decoded tensors and the restated partial sums; never modified."""
    out = {}
    for values, (ref, *_rest) in WIRES.items():
        for k, _mode, _make in CASES:
            S = slot_wire_bytes("topk", k, values)
            recv = np.concatenate([np.concatenate([ref.encode_tensor(t, k)[0] for t in g])
                                   for g in (special(21), tied(22))])
            slots, _ = ref.reduce_slots(recv, 2, recv.size // (2 * S), 2, k)
            slots[3 * S:4 * S] = 0
            vals = _decoded(ref, slots, k)
            assert np.isnan(np.concatenate(vals)).any() and not vals[3].any()
            out[values, k] = dict(slots=slots, vals=vals, parts=cr.tree_partials(vals))
    return out


@VALUES
@ALIGN
@pytest.mark.parametrize("sumsq", [False, True], ids=["no_partials", "partials"])
@pytest.mark.parametrize("k,mode", [c[:2] for c in CASES], ids=[f"k{c[0]}-{c[1]}" for c in CASES])
def test_unpack_avg_topk_matches_the_restatement(averaged, k, mode, sumsq, misaligned, values):
    unpack, want = WIRES[values][2], averaged[values, k]
    rig = _Rig(k, values, misaligned, mode)
    rig.slots.copy_(torch.from_numpy(want["slots"]))
    partials = torch.full((rig.nch,), PART_SENTINEL, dtype=torch.float64, device=DEV)

    def one(b, s):
        unpack(rig.tree, b, s, k, SLOT_GRAD, partials if sumsq else None)
        if b != ALL:  # a bucket launch writes exactly its chunk range of the partial sums
            c0, c1 = rig.tree.bucket_chunks[b]
            p = partials.cpu().numpy()
            assert (p[:c0] == PART_SENTINEL).all() and (p[c0:c1] != PART_SENTINEL).all() == sumsq

    rig.launch(one)
    for d, v in zip(rig.grads, want["vals"]):
        assert tk.same_bits(d.cpu().numpy(), v), v.size
    rig.guards_hold()
    assert rig.slots.cpu().numpy().tobytes() == want["slots"].tobytes()  # only read
    got = partials.cpu().numpy()
    if sumsq:  # the restatement's, and dl_grad_sumsq's on the destination afterwards
        again = torch.full_like(partials, PART_SENTINEL)
        K.grad_sumsq(rig.tree, ALL, SLOT_GRAD, again)
        assert tk.same_bits(got, want["parts"]) and tk.same_bits(again.cpu().numpy(), got)
        assert np.isnan(got).any()
    else:
        assert (got == PART_SENTINEL).all()
    rig.tree.close()


# ---- 3: GradSync, one replica ----------------------------------------------------------------
def _params(grads):
    ps = [torch.nn.Parameter(torch.zeros(g.size, device=DEV)) for g in grads]
    _set_grads(ps, grads)
    return ps


def _set_grads(ps, grads):
    for p, g in zip(ps, grads):
        p.grad = torch.from_numpy(g).to(DEV)  # a fresh tensor every step


@VALUES
def test_gradsync_one_replica_matches_the_restatement(values):
    """encode with the residual -> the reduce of the region onto itself, no residual -> decode."""
    ref, ps = WIRES[values][0], _params(groupwise(40))
    gs = GradSync(ps, None, 1, wire_dtype="topk", topk=64, topk_values=values, bucket_cap_elems=CAP)
    assert gs.world_size == 1 and gs.error_feedback and gs.tree.n_buckets >= 3
    res = [np.zeros(n, dtype=F) for n in NUMELS]
    for s in (1, 2):  # the second sync carries a residual
        g = tied(40 + s)
        _set_grads(ps, g)
        assert gs.sync() is None
        torch.cuda.synchronize()
        enc = [ref.encode_tensor(x, 64, r) for x, r in zip(g, res)]
        res = [r for _, r in enc]
        slots = np.concatenate([e for e, _ in enc])
        want = _decoded(ref, ref.reduce_slots(slots, 1, gs.tree.n_chunks, 1, 64)[0], 64)
        for t, (p, w) in enumerate(zip(ps, want)):
            assert p.grad.cpu().numpy().tobytes() == w.tobytes(), (s, t)
    st = gs.q8_ef_state()
    enc = st["encode"].cpu().numpy()
    for t, o in enumerate(gs.tree.seg_off[:-1]):
        assert enc[int(o):int(o) + NUMELS[t]].tobytes() == res[t].tobytes(), t
    assert st["reduce"] == [] and enc.any()
    gs.close()


@VALUES
@pytest.mark.parametrize("factor", [0.5, 2.0], ids=["clips", "does_not_clip"])
def test_gradsync_topk_with_max_norm_equals_sync_then_clip(factor, values):
    pa, pb = _params(groupwise(50)), _params(groupwise(50))
    kw = dict(wire_dtype="topk", topk_values=values, bucket_cap_elems=CAP)
    ga, gb = GradSync(pa, None, 1, **kw), GradSync(pb, None, 1, **kw)
    for s in (1, 2):
        g = groupwise(50 + s)
        _set_grads(pa, g)
        _set_grads(pb, g)
        assert gb.sync() is None
        torch.cuda.synchronize()
        norm0, _ = cr.norm_and_coef([p.grad.cpu().numpy() for p in pb], 1.0)
        got = ga.sync(float(norm0) * factor)
        want = utils.clip_grad_norm_(pb, float(norm0) * factor)
        torch.cuda.synchronize()
        assert np.float32(got.item()).tobytes() == np.float32(want.item()).tobytes() == norm0.tobytes()
        for a, b in zip(pa, pb):
            assert torch.equal(a.grad.view(torch.int32), b.grad.view(torch.int32)), s
    assert torch.equal(ga.q_residual.view(torch.int32), gb.q_residual.view(torch.int32))
    ga.close()
    gb.close()


# ---- 4: two gloo ranks on the one GPU, through TrainingComm ----------------------------------
NUMELS_DP = NUMELS + [5]  # an odd chunk count in DPSync's one bucket: a padding slot at two peers


def _worker(rank, world, port):
    for p in (PKG, REPO, os.path.join(REPO, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(DILOCO_DP_BACKEND="gloo", DILOCO_COLLECTIVE_READ_TIMEOUT="10")
    for v in [v for v in os.environ if v.startswith("DILOCO_DP_") and v != "DILOCO_DP_BACKEND"]:
        os.environ.pop(v)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank,
                            world_size=world)
    from diloco_amd import comm
    from diloco_amd.world import World

    assert (comm.DP_WIRE, comm.DP_TOPK, comm.DP_TOPK_VALUES, comm.DP_TOPK_EF) == ("f32", 64, "f32", True)
    tc = comm.TrainingComm(World.from_default_group(1), (1, 1, 32), None)
    counts = [sum(-(-n // tk.CHUNK) for n in NUMELS_DP)]  # DPSync's default cap: one bucket
    assert counts[0] % 2
    for values, (ref, *_rest) in WIRES.items():
        comm.DP_WIRE, comm.DP_TOPK, comm.DP_TOPK_VALUES = "topk", 32, values  # the knobs, patched
        model = torch.nn.Module()
        model.ps = torch.nn.ParameterList(
            [torch.nn.Parameter(torch.zeros(n, device=DEV)) for n in NUMELS_DP])
        ex = ref.TopkExchange(NUMELS_DP, counts, world, 32)
        for s in (1, 2):
            by_rank = [groupwise(100 * s + r, NUMELS_DP) for r in range(world)]
            _set_grads(list(model.parameters()), by_rank[rank])
            assert tc.sync_gradients(model) is None
            torch.cuda.synchronize()
            got = np.concatenate([p.grad.cpu().numpy() for p in model.parameters()])
            # the restatement's bytes on every rank, so byte-identical across the ranks
            assert got.tobytes() == np.concatenate(ex.average(by_rank)).tobytes(), (values, s)
        gs = tc.dp._grad_syncs[id(model)]
        assert (gs.topk, gs.topk_values, gs.error_feedback, gs.local) == (32, values, True, False)
        assert [c1 - c0 for c0, c1 in gs.tree.bucket_chunks] == counts
        st = gs.q8_ef_state()
        enc = st["encode"].cpu().numpy()
        enc = np.concatenate([enc[int(o):int(o) + n] for o, n in zip(gs.tree.seg_off, NUMELS_DP)])
        assert tk.same_bits(enc, np.concatenate(ex.enc[rank])) and enc.any()
        red = np.concatenate([a.cpu().numpy() for a in st["reduce"]])
        assert tk.same_bits(red, np.concatenate([r[rank] for r in ex.red])) and red.any()
        gs.load_q8_ef_state(None)
        assert not gs.q_residual.any() and not any(r.any() for r in gs.q_residual_red)
        gs.load_q8_ef_state(st)
        again = gs.q8_ef_state()
        assert torch.equal(again["encode"].view(torch.int32), st["encode"].view(torch.int32))
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                   for a, b in zip(again["reduce"], st["reduce"]))
    dist.barrier()
    dist.destroy_process_group()


def test_training_comm_topk_wire_two_peers_on_gpu():
    """Two gloo processes on the one GPU, TrainingComm.sync_gradients with the DILOCO_DP_TOPK*
    knobs patched, both value formats, two steps each: dl_gather_topk[_fp4] -> all_to_all ->
    dl_topk[_fp4]_reduce -> all_gather -> dl_unpack_avg_topk[_fp4] (asserted inside each rank; a
    failing rank fails the spawn)."""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mp.spawn(_worker, args=(2, port), nprocs=2, join=True)
