"""The fp4 (MXFP4) wire of the per-step DP gradient sync, on the GPU: dl_gather_fp4 and
dl_unpack_avg_fp4 against the checker backend (tests/gradsync_fp4_oracle_kernels.py:
tests/fp4_restatement.py, tests/clip_restatement.py) bit for bit, NaNs by position; GradSync,
DPSync and TrainingComm on top of them against the exchange composed by hand.

The tree (tests/gradsync_fp4_inputs.py) has a 1-element chunk, tails under 4 and under 32, a chunk
one short of full, a full one, a one-element spill and a three-chunk tensor; bucket cap 4096
splits it into several buckets. Gradient tensors are views into one sentinel-filled buffer with
guard floats between them, 16-B aligned (the float4 rows, a group is 8 lanes) or one float off
(the 32-lane group path, scalar stores). Slots start as 0xFF between two guard slots, the
residual's padding as a NaN bit pattern."""
import os
import socket
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import clip_restatement as cr
import fp4_restatement as fp4
import gradsync_fp4_footprint as gf
from conftest import PKG, REPO
from diloco_amd import _lib, utils
from diloco_amd.gradsync import GradSync
from diloco_amd.kernels import HipKernels
from diloco_amd.plan import SLOT_GRAD, SLOT_INNER, PackedTree
from gradsync_fp4_inputs import CAP, NUMELS, groupwise, special
from gradsync_fp4_oracle_kernels import GradSyncFp4OracleKernels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
SLOT, CHUNK = fp4.SLOT, fp4.CHUNK
ALL = _lib.ALL_BUCKETS
NAN_BITS = 0x7F8BEEF5  # a NaN bit pattern: the residual arena's padding before every run
GUARD = 4  # floats before and after every tensor of the guarded layout
SENTINEL = F(-123.25)
K = HipKernels()
REF = GradSyncFp4OracleKernels()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _small(seed):
    """A residual an earlier step could have left: a hundredth of the gradients' magnitudes."""
    return [(x * F(0.01)).astype(F) for x in groupwise(seed)]


class _Rig:
    """One tree on the device and its host twin on the checker backend."""

    def __init__(self, misaligned=False, max_blocks=0):
        self.tree = PackedTree(NUMELS, CAP)
        self.cpu = REF.tree(NUMELS, None, CAP)
        assert self.tree.n_buckets >= 3 and self.tree.bucket_chunks == self.cpu.bucket_chunks
        assert self.tree.total == self.cpu.total and self.tree.n_chunks == len(self.cpu.chunks)
        if max_blocks:
            self.tree.tune(max_blocks)  # a workgroup walks several chunks: its LDS is reused
        self.nch = self.tree.n_chunks
        self.offs = [int(o) for o in self.tree.seg_off[:-1]]
        self.pad = np.ones(self.tree.total, dtype=bool)
        for o, n in zip(self.offs, NUMELS):
            self.pad[o:o + n] = False
        self.at, at = [], GUARD + (1 if misaligned else 0)
        for n in NUMELS:
            self.at.append(at)
            at += n + GUARD + (-(n + GUARD)) % 4
        self.base = torch.full((at + GUARD,), float(SENTINEL), dtype=torch.float32, device=DEV)
        assert self.base.data_ptr() % 16 == 0
        self.grads = [self.base[a:a + n] for a, n in zip(self.at, NUMELS)]
        assert all(g.data_ptr() % 16 == (4 if misaligned else 0) for g in self.grads)
        self.guard = np.ones(self.base.numel(), dtype=bool)
        for a, n in zip(self.at, NUMELS):
            self.guard[a:a + n] = False
        self.tree.bind(SLOT_GRAD, self.grads, _stream())
        res0 = np.zeros(self.tree.total, dtype=np.uint32)
        res0[self.pad] = NAN_BITS
        self.resid = torch.from_numpy(res0.view(F).copy()).to(DEV)
        # a guard slot before and after the tree's slots
        self.all_slots = torch.full(((self.nch + 2) * SLOT,), 0xFF, dtype=torch.uint8, device=DEV)
        self.slots = self.all_slots[SLOT:-SLOT]
        assert self.slots.data_ptr() % 16 == 0
        self.h_grads = [torch.zeros(n) for n in NUMELS]
        self.h_resid = torch.from_numpy(res0.view(F).copy())
        self.h_slots = torch.zeros(self.nch * SLOT, dtype=torch.uint8)
        REF.bind(self.cpu, SLOT_GRAD, self.h_grads, None)

    def feed(self, grads, resid=None):
        for g, d, h in zip(grads, self.grads, self.h_grads):
            h.copy_(torch.from_numpy(g))
            d.copy_(h)
        if resid is not None:
            for o, r in zip(self.offs, resid):
                self.h_resid[o:o + r.size] = torch.from_numpy(r)
            self.resid.copy_(self.h_resid)

    def bucket_slots(self, buf, b):
        c0, c1 = self.tree.bucket_chunks[b]
        return buf[c0 * SLOT:c1 * SLOT]

    def guards_hold(self, what):
        s = self.all_slots.cpu().numpy()
        assert (s[:SLOT] == 0xFF).all() and (s[-SLOT:] == 0xFF).all(), (what, "guard slots")
        assert (self.base.cpu().numpy()[self.guard] == SENTINEL).all(), (what, "guard floats")

    def encode(self, feedback, whole, what):
        """The checker first, then the device: whole-tree, or bucket by bucket from the last
        one, checking after every launch that the slots not launched yet still hold 0xFF."""
        REF.gather_fp4(self.cpu, ALL, SLOT_GRAD, self.h_resid if feedback else None, self.h_slots)
        self.all_slots.fill_(0xFF)
        want = self.h_slots.numpy()
        resid = self.resid if feedback else None
        if whole:
            K.gather_fp4(self.tree, ALL, SLOT_GRAD, resid, self.slots)
        else:
            for b in reversed(range(self.tree.n_buckets)):
                K.gather_fp4(self.tree, b, SLOT_GRAD, resid, self.bucket_slots(self.slots, b))
                got = self.slots.cpu().numpy()
                at = self.tree.bucket_chunks[b][0] * SLOT
                assert (got[:at] == 0xFF).all(), (what, "other buckets' slots", b)
                assert got[at:].tobytes() == want[at:].tobytes(), (what, "slots", b)
        torch.cuda.synchronize()
        got = self.slots.cpu().numpy()
        # every byte of the launched slots is overwritten: the checker's slots started as zeros
        assert got.tobytes() == want.tobytes(), (what, "slots", int((got != want).sum()))
        for c, (_seg, _o, n, _po) in enumerate(self.cpu.chunks):
            s = got[c * SLOT:(c + 1) * SLOT]
            assert not s[-(-n // 32):fp4.N_GROUPS].any(), (what, "scales past the length", c)
            assert not s[fp4.N_GROUPS + -(-n // 2):].any(), (what, "nibbles past the length", c)
        got_r, want_r = self.resid.cpu().numpy(), self.h_resid.numpy()
        assert fp4.same_bits(got_r[~self.pad], want_r[~self.pad]), (what, "residual")
        assert (got_r.view(np.uint32)[self.pad] == NAN_BITS).all(), (what, "residual padding")
        self.guards_hold(what)
        # the gradients are only read
        assert fp4.same_bits(np.concatenate([g.cpu().numpy() for g in self.grads]),
                             np.concatenate([h.numpy() for h in self.h_grads])), (what, "grads")

    def close(self):
        self.tree.close()


LAUNCHES = [(whole, mb) for whole in (True, False) for mb in (0, 2)]
LAUNCH_IDS = [f"{'tree' if w else 'buckets'}-max_blocks_{mb}" for w, mb in LAUNCHES]
ALIGN = pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
LAUNCH = pytest.mark.parametrize("launch", LAUNCHES, ids=LAUNCH_IDS)


# ---- 1: the encoder --------------------------------------------------------------------------
@ALIGN
@LAUNCH
def test_gather_fp4_matches_the_checker(launch, misaligned):
    whole, mb = launch
    rig = _Rig(misaligned, mb)
    rig.feed(special(5))
    rig.encode(False, whole, "plain")
    e = rig.h_slots.numpy().reshape(-1, SLOT)[:, :fp4.N_GROUPS]
    assert (e == 255).sum() == 2 and len(np.unique(e)) > 8  # a NaN and an Inf group; many scales
    assert not rig.resid.cpu().numpy()[~rig.pad].any()  # no residual without error feedback
    rig.close()


@ALIGN
@LAUNCH
def test_gather_fp4_with_residual_matches_the_checker_over_three_steps(launch, misaligned):
    """The residual of one step feeds the next (a NaN group's stays NaN, position for position)."""
    whole, mb = launch
    rig = _Rig(misaligned, mb)
    for s in (1, 2, 3):
        rig.feed(special(10 + s))
        rig.encode(True, whole, s)
        r = rig.resid.cpu().numpy()[~rig.pad]
        # most elements are below half a step: they live on in the residual
        assert (np.nan_to_num(r) != 0).mean() > 0.5
    rig.close()


@ALIGN
@pytest.mark.parametrize("feedback", [False, True], ids=["plain", "ef"])
def test_gather_fp4_equals_delta_fp4_with_a_zero_inner(feedback, misaligned):
    """outer bound to the same values, inner = +0: byte for byte, the residual too."""
    rig = _Rig(misaligned)
    g = special(7)
    rig.feed(g, _small(8) if feedback else None)
    theta = torch.zeros(rig.tree.total, device=DEV)
    for o, x in zip(rig.offs, g):
        theta[o:o + x.size] = torch.from_numpy(x).to(DEV)
    zeros = torch.zeros(rig.base.numel(), device=DEV)
    rig.tree.bind(SLOT_INNER, [zeros[a:a + n] for a, n in zip(rig.at, NUMELS)], _stream())
    r_a = rig.resid if feedback else None
    r_b = rig.resid.clone() if feedback else None
    other = torch.full_like(rig.all_slots, 0xFF)
    K.gather_fp4(rig.tree, ALL, SLOT_GRAD, r_a, rig.slots)
    K.delta_fp4(rig.tree, ALL, SLOT_INNER, theta, r_b, other[SLOT:-SLOT])
    torch.cuda.synchronize()
    assert torch.equal(rig.all_slots, other)
    if feedback:
        assert fp4.same_bits(r_a.cpu().numpy()[~rig.pad], r_b.cpu().numpy()[~rig.pad])
        assert (r_a.cpu().numpy().view(np.uint32)[rig.pad] == NAN_BITS).all()
    rig.close()


# ---- 2: the decoder --------------------------------------------------------------------------
PART_SENTINEL = -7.0


@pytest.fixture(scope="module")
def averaged():
    """Slots as an exchange leaves them (the restatement's encoder, then its reduce over two
    peers; a NaN and an Inf group among them), their decoded values per tensor and the restated
    partial sums; never modified."""
    recv = np.concatenate([np.concatenate([fp4.encode_delta(t)[0] for t in g])
                           for g in (special(21), groupwise(22))])
    m = recv.size // (2 * SLOT)
    slots, _ = fp4.reduce_slots(recv, 2, m, 2)
    vals = fp4.decode_tensors(slots, NUMELS)
    assert sum(np.isnan(v).sum() for v in vals) == 64
    return dict(slots=slots, vals=vals, parts=cr.tree_partials(vals))


def _check_decoded(rig, vals, what):
    got = rig.base.cpu().numpy()
    for a, n, v in zip(rig.at, NUMELS, vals):
        assert fp4.same_bits(got[a:a + n], v), (what, "dst", n)
    assert (got[rig.guard] == SENTINEL).all(), (what, "guard floats")


@ALIGN
@LAUNCH
@pytest.mark.parametrize("sumsq", [False, True], ids=["no_partials", "partials"])
def test_unpack_avg_fp4_matches_the_checker(averaged, sumsq, launch, misaligned):
    whole, mb = launch
    rig = _Rig(misaligned, mb)
    rig.slots.copy_(torch.from_numpy(averaged["slots"]))
    rig.h_slots.copy_(torch.from_numpy(averaged["slots"]))
    nch = rig.nch
    partials = torch.full((nch,), PART_SENTINEL, dtype=torch.float64, device=DEV)
    arg = partials if sumsq else None
    if whole:
        K.unpack_avg_fp4(rig.tree, ALL, rig.slots, SLOT_GRAD, arg)
    else:
        for b in reversed(range(rig.tree.n_buckets)):
            K.unpack_avg_fp4(rig.tree, b, rig.bucket_slots(rig.slots, b), SLOT_GRAD, arg)
            c0, c1 = rig.tree.bucket_chunks[b]
            p = partials.cpu().numpy()
            # a bucket launch writes exactly its chunk range; the others keep the sentinel
            assert (p[:c0] == PART_SENTINEL).all(), b
            assert (p[c0:c1] != PART_SENTINEL).all() == sumsq, b
    torch.cuda.synchronize()
    _check_decoded(rig, averaged["vals"], "decoder")
    s = rig.all_slots.cpu().numpy()
    assert s[SLOT:-SLOT].tobytes() == averaged["slots"].tobytes()  # only read
    assert (s[:SLOT] == 0xFF).all() and (s[-SLOT:] == 0xFF).all()
    h_part = torch.full((nch,), PART_SENTINEL, dtype=torch.float64)
    REF.unpack_avg_fp4(rig.cpu, ALL, rig.h_slots, SLOT_GRAD, h_part if sumsq else None)
    for h, v in zip(rig.h_grads, averaged["vals"]):
        assert fp4.same_bits(h.numpy(), v)
    got = partials.cpu().numpy()
    if not sumsq:
        assert (got == PART_SENTINEL).all()
    else:
        # the checker backend, the restatement, and dl_grad_sumsq on the destination afterwards
        assert fp4.same_bits(got, h_part.numpy())
        assert fp4.same_bits(got, averaged["parts"])
        again = torch.full((nch,), PART_SENTINEL, dtype=torch.float64, device=DEV)
        K.grad_sumsq(rig.tree, ALL, SLOT_GRAD, again)
        assert fp4.same_bits(again.cpu().numpy(), got) and np.isnan(got).sum() == 2
    rig.close()


def test_argument_errors_are_raised_before_any_launch():
    tree = PackedTree([10, 20])
    s = _stream()
    buf = torch.zeros(2 * SLOT, device=DEV)
    a = buf.data_ptr()
    for name, args in (("dl_gather_fp4", (tree.handle, ALL, SLOT_GRAD, None, a)),
                       ("dl_unpack_avg_fp4", (tree.handle, ALL, a, SLOT_GRAD, a))):
        with pytest.raises(_lib.DilocoHipError, match="not bound") as e:
            _lib.call(name, *args, s)
        assert e.value.code == -2 and name in str(e.value)  # DL_E_STATE
    tree.bind(SLOT_GRAD, [torch.zeros(10, device=DEV), torch.zeros(20, device=DEV)], s)
    for name, args, msg in [
            ("dl_gather_fp4", (tree.handle, ALL, SLOT_GRAD, None, None), "slots is null"),
            ("dl_gather_fp4", (tree.handle, ALL, SLOT_GRAD, None, a + 8), "slots not 16-B"),
            ("dl_gather_fp4", (tree.handle, ALL, SLOT_GRAD, a + 4, a), "residual not 16-B"),
            ("dl_gather_fp4", (tree.handle, 5, SLOT_GRAD, None, a), "bucket 5"),
            ("dl_gather_fp4", (tree.handle, ALL, 99, None, a), "slot 99"),
            ("dl_unpack_avg_fp4", (tree.handle, ALL, None, SLOT_GRAD, None), "slots is null"),
            ("dl_unpack_avg_fp4", (tree.handle, ALL, a + 8, SLOT_GRAD, None), "slots not 16-B"),
            ("dl_unpack_avg_fp4", (tree.handle, ALL, a, SLOT_GRAD, a + 4), "partials not 8-B"),
            ("dl_unpack_avg_fp4", (tree.handle, ALL, a, 99, None), "slot 99")]:
        with pytest.raises(_lib.DilocoHipError, match=msg):
            _lib.call(name, *args, s)
    torch.cuda.synchronize()
    assert not buf.any()  # nothing was launched
    tree.close()


# ---- 3: write footprints (tests/footprint.py's arena, sentinels and comparison) --------------
@pytest.mark.parametrize("row", list(gf.ROWS))
def test_footprint(row):
    """Both sentinels, tensors 0, 1 and mixed 0-3 elements off a 16-B boundary, whole-tree and
    bucket by bucket, grid caps 0, 1, 2 and 5, two consecutive launches: after every launch every
    byte of every buffer equals the CPU reference's."""
    for case in gf.ROWS[row]():
        gf.run_case(case, K, DEV, grids=gf.fpt.GRIDS)


# ---- 4: GradSync, one replica ----------------------------------------------------------------
def _params(grads):
    ps = []
    for g in grads:
        p = torch.nn.Parameter(torch.zeros(g.size, device=DEV))
        p.grad = torch.from_numpy(g).to(DEV)
        ps.append(p)
    return ps


def _set_grads(ps, grads):
    for p, g in zip(ps, grads):
        p.grad = torch.from_numpy(g).to(DEV)  # a fresh tensor every step


@pytest.mark.parametrize("feedback", [False, True], ids=["plain", "ef"])
def test_gradsync_one_replica_matches_the_restatement(feedback):
    """encode -> dl_fp4_reduce of the region onto itself (the identity) -> decode, three syncs,
    against Fp4Exchange at n = 1."""
    ps = _params(groupwise(40))
    gs = GradSync(ps, None, 1, wire_dtype="fp4", bucket_cap_elems=CAP, error_feedback=feedback)
    assert gs.world_size == 1 and gs.fp4 and gs.tree.n_buckets >= 3
    counts = [c1 - c0 for c0, c1 in gs.tree.bucket_chunks]
    ex = fp4.Fp4Exchange(NUMELS, counts, 1, ef=feedback)
    for s in (1, 2, 3):
        g = groupwise(40 + s)
        _set_grads(ps, g)
        assert gs.sync() is None
        torch.cuda.synchronize()
        want = ex.average([g])
        for t, (p, w) in enumerate(zip(ps, want)):
            assert p.grad.cpu().numpy().tobytes() == w.tobytes(), (s, t)
    st = gs.q8_ef_state()
    if feedback:
        assert st["reduce"] == [] and bool(st["encode"].any())
        enc = st["encode"].cpu().numpy()
        for t, o in enumerate(gs.tree.seg_off[:-1]):
            assert enc[int(o):int(o) + NUMELS[t]].tobytes() == ex.enc[0][t].tobytes(), t
        gs.load_q8_ef_state(None)
        assert not bool(gs.q_residual.any())
    else:
        assert st is None
    gs.close()


@pytest.mark.parametrize("factor", [0.5, 2.0], ids=["clips", "does_not_clip"])
def test_gradsync_fp4_with_max_norm_equals_sync_then_clip(factor):
    g = groupwise(50)
    pa, pb = _params(g), _params(g)
    kw = dict(wire_dtype="fp4", bucket_cap_elems=CAP, error_feedback=True)
    ga, gb = GradSync(pa, None, 1, **kw), GradSync(pb, None, 1, **kw)
    for s in (1, 2):
        g = groupwise(50 + s)
        _set_grads(pa, g)
        _set_grads(pb, g)
        assert gb.sync() is None
        torch.cuda.synchronize()
        unclipped = [p.grad.clone() for p in pb]
        norm0, _ = cr.norm_and_coef([u.cpu().numpy() for u in unclipped], 1.0)
        max_norm = float(norm0) * factor
        got = ga.sync(max_norm)
        want = utils.clip_grad_norm_(pb, max_norm)
        torch.cuda.synchronize()
        assert got.dtype == torch.float32 and got.dim() == 0
        assert np.float32(got.item()).tobytes() == np.float32(want.item()).tobytes(), s
        assert np.float32(got.item()).tobytes() == norm0.tobytes(), s
        for a, b in zip(pa, pb):
            assert torch.equal(a.grad.view(torch.int32), b.grad.view(torch.int32)), s
        # the clip scaled the decoded values exactly when the norm exceeded max_norm
        assert all(torch.equal(p.grad, u) for p, u in zip(pb, unclipped)) == (factor > 1)
    assert torch.equal(ga.q_residual.view(torch.int32), gb.q_residual.view(torch.int32))
    ga.close()
    gb.close()


# ---- 5: two gloo ranks on the one GPU, through TrainingComm ----------------------------------
STEPS = 3
NUMELS_DP = NUMELS + [5]  # an odd chunk count in DPSync's one bucket: a padding slot at two peers


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out):
    for p in (PKG, REPO, os.path.join(REPO, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from datetime import timedelta

    os.environ["DILOCO_DP_BACKEND"] = "gloo"
    for v in ("DILOCO_DP_EXCHANGE", "DILOCO_DP_WIRE", "DILOCO_DP_Q8_EF", "DILOCO_DP_FP4_EF"):
        os.environ.pop(v, None)
    os.environ["DILOCO_COLLECTIVE_READ_TIMEOUT"] = "10"  # every collective has its own limit
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank,
                            world_size=world, timeout=timedelta(seconds=30))
    from diloco_amd import comm
    from diloco_amd.world import World

    assert comm.DP_WIRE == "f32" and comm.DP_FP4_EF is False and comm.dp_backend() == "gloo"
    comm.DP_WIRE, comm.DP_FP4_EF = "fp4", True  # the knobs, patched
    model = torch.nn.Module()
    model.ps = torch.nn.ParameterList(
        [torch.nn.Parameter(torch.zeros(n, device=DEV)) for n in NUMELS_DP])
    tc = comm.TrainingComm(World.from_default_group(1), (1, 1, 32), None)
    rec, ex = {}, None
    for s in range(1, STEPS + 2):
        by_rank = [groupwise(100 * s + r, NUMELS_DP) for r in range(world)]
        for p, g in zip(model.parameters(), by_rank[rank]):
            p.grad = torch.from_numpy(g).to(DEV)  # reallocated every step
        if ex is None:
            counts = [sum(-(-n // CHUNK) for n in NUMELS_DP)]  # DPSync's default cap: one bucket
            ex = fp4.Fp4Exchange(NUMELS_DP, counts, world, ef=True)
        want = ex.average(by_rank)
        if s <= STEPS:
            assert tc.sync_gradients(model) is None
        else:  # the last step clips too: sync(max_norm) through the same call
            norm0, _ = cr.norm_and_coef(want, 1.0)
            norm, coef, want = cr.clip(want, float(norm0) * 0.5)
            got = tc.sync_gradients(model, float(norm0) * 0.5)
            rec["norm"] = np.array([np.float32(got.item()), norm])
            assert coef < 1
        torch.cuda.synchronize()
        gs = next(iter(tc.dp._grad_syncs.values()))
        assert gs.fp4 and gs.error_feedback and not gs.local
        assert [c1 - c0 for c0, c1 in gs.tree.bucket_chunks] == counts
        rec[f"grad_s{s}"] = np.concatenate([p.grad.cpu().numpy() for p in model.parameters()])
        rec[f"ref_s{s}"] = np.concatenate(want)
    rec["counts"] = np.array(counts)
    st = gs.q8_ef_state()
    rec["encode_nonzero"] = np.array(bool(st["encode"].any()))
    rec["reduce"] = np.concatenate([a.cpu().numpy() for a in st["reduce"]])
    rec["ref_reduce"] = np.concatenate([ex.red[b][rank] for b in range(len(ex.red))])
    np.savez(os.path.join(out, f"r{rank}.npz"), **rec)
    dist.barrier()
    dist.destroy_process_group()


def test_training_comm_fp4_wire_two_peers_on_gpu():
    """Two gloo processes on the one GPU, TrainingComm.sync_gradients with comm.DP_WIRE patched
    to fp4 and error feedback on, three steps and a fourth with max_norm: dl_gather_fp4 ->
    all_to_all -> dl_fp4_reduce -> all_gather -> dl_unpack_avg_fp4. Both ranks end with the same
    bytes, equal to the exchange composed by hand."""
    out = tempfile.mkdtemp(prefix="dl_gradsync_fp4_")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    recs = [dict(np.load(os.path.join(out, f"r{r}.npz"))) for r in range(2)]
    assert any(int(c) % 2 for c in recs[0]["counts"])
    for rec in recs:
        for s in range(1, STEPS + 2):
            got, want = rec[f"grad_s{s}"], rec[f"ref_s{s}"]
            assert got.tobytes() == want.tobytes(), (s, int((got != want).sum()))
            assert got.tobytes() == recs[0][f"grad_s{s}"].tobytes(), s
        assert rec["norm"][0].tobytes() == rec["norm"][1].tobytes()
        assert bool(rec["encode_nonzero"])
        assert rec["reduce"].tobytes() == rec["ref_reduce"].tobytes() and rec["reduce"].any()
