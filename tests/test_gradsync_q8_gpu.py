"""The int8 wire of the per-step DP gradient sync, on the GPU: dl_gather_q8, dl_gather_q8_ef and
dl_unpack_avg_q8 against the checker backend (tests/gradsync_q8_oracle_kernels.py: the C oracle's
quantiser, tests/q8_ef_restatement.py, tests/clip_restatement.py) bit for bit, NaNs by position;
GradSync and DPSync on top of them against the exchange composed by hand.

The tree has a 1-element chunk, tails under 4, a chunk one short of full, a full one, one that
spills a single element into a second chunk, and a three-chunk tensor; bucket cap 4096 splits it
into several buckets. Gradient tensors sit in their own allocations (16-B aligned: the vector
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

import clip_restatement as cr
import q8_ef_restatement as ef
from conftest import PKG, REPO
from diloco_amd import _lib, utils
from diloco_amd.gradsync import GradSync
from diloco_amd.kernels import HipKernels
from diloco_amd.plan import SLOT_GRAD, PackedTree
from gradsync_q8_oracle_kernels import GradSyncQ8OracleKernels
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
NUMELS = [1, 3, 257, 4095, 4096, 4097, 8197]
CAP = 4096
SLOT, HDR, CHUNK = oracle.Q8_SLOT, oracle.Q8_HDR, oracle.CHUNK
ALL = _lib.ALL_BUCKETS
NAN_BITS = 0x7F8BEEF5  # a NaN bit pattern: the residual arena's padding before every run
GUARD = 4  # floats before and after every tensor of the guarded layout
K = HipKernels()
REF = GradSyncQ8OracleKernels()


def _grads(seed, numels=NUMELS):
    """One element of ~1 per 1500 and ~1e-3 elsewhere: most elements quantise to 0 and live on
    in the residual."""
    rng = np.random.default_rng(seed)
    out = []
    for n in numels:
        g = (1e-3 * rng.standard_normal(n)).astype(F)
        g[::1500] = 1.0 + rng.random(g[::1500].size).astype(F)
        out.append(g)
    return out


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Rig:
    """One tree on the device and its host twin on the checker backend. The gradient tensors
    are views into one buffer of a sentinel value, GUARD floats apart, at 16-B boundaries or
    one float past them; slots start as 0xFF, the residual's padding as a NaN pattern."""

    def __init__(self, misaligned=False, max_blocks=0):
        self.tree = PackedTree(NUMELS, CAP)
        self.cpu = REF.tree(NUMELS, None, CAP)
        assert self.tree.n_buckets >= 2 and self.tree.bucket_chunks == self.cpu.bucket_chunks
        assert self.tree.total == self.cpu.total and self.tree.n_chunks == len(self.cpu.chunks)
        if max_blocks:
            self.tree.tune(max_blocks)  # a workgroup walks several chunks: LDS is reused
        self.offs = [int(o) for o in self.tree.seg_off[:-1]]
        self.pad = np.ones(self.tree.total, dtype=bool)
        for o, n in zip(self.offs, NUMELS):
            self.pad[o:o + n] = False
        self.at, at = [], GUARD + (1 if misaligned else 0)
        for n in NUMELS:
            self.at.append(at)
            at += n + GUARD + (-(n + GUARD)) % 4
        self.base = torch.full((at + GUARD,), -123.25, dtype=torch.float32, device=DEV)
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
        self.slots = torch.full((self.tree.n_chunks * SLOT,), 0xFF, dtype=torch.uint8, device=DEV)
        self.h_grads = [torch.zeros(n) for n in NUMELS]
        self.h_resid = torch.from_numpy(res0.view(F).copy())
        self.h_slots = torch.zeros(self.tree.n_chunks * SLOT, dtype=torch.uint8)
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

    def encode(self, feedback, whole, what):
        """The checker first, then the device: whole-tree, or bucket by bucket from the last
        one, checking after every launch that the slots not launched yet still hold 0xFF."""
        if feedback:
            REF.gather_q8_ef(self.cpu, ALL, SLOT_GRAD, self.h_resid, self.h_slots)
        else:
            REF.gather_q8(self.cpu, ALL, SLOT_GRAD, self.h_slots)
        self.slots.fill_(0xFF)
        want = self.h_slots.numpy()

        def launch(b, slots):
            if feedback:
                K.gather_q8_ef(self.tree, b, SLOT_GRAD, self.resid, slots)
            else:
                K.gather_q8(self.tree, b, SLOT_GRAD, slots)

        if whole:
            launch(ALL, self.slots)
        else:
            for b in reversed(range(self.tree.n_buckets)):
                launch(b, self.bucket_slots(self.slots, b))
                got = self.slots.cpu().numpy()
                at = self.tree.bucket_chunks[b][0] * SLOT
                assert (got[:at] == 0xFF).all(), (what, "other buckets' slots", b)
                assert got[at:].tobytes() == want[at:].tobytes(), (what, "slots", b)
        torch.cuda.synchronize()
        got = self.slots.cpu().numpy()
        # every byte of the launched slots is overwritten: the checker's slots started as zeros
        assert got.tobytes() == want.tobytes(), (what, "slots", int((got != want).sum()))
        for c, (_seg, _o, n, _po) in enumerate(self.cpu.chunks):
            assert not got[c * SLOT + HDR + n:(c + 1) * SLOT].any(), (what, "payload tail", c)
            assert not got[c * SLOT + 4:c * SLOT + HDR].any(), (what, "header", c)
        got_r, want_r = self.resid.cpu().numpy(), self.h_resid.numpy()
        assert ef.same_bits(got_r[~self.pad], want_r[~self.pad]), (what, "residual")
        assert (got_r.view(np.uint32)[self.pad] == NAN_BITS).all(), (what, "residual padding")
        # the gradients are only read
        assert ef.same_bits(np.concatenate([g.cpu().numpy() for g in self.grads]),
                            np.concatenate([h.numpy() for h in self.h_grads])), (what, "grads")

    def close(self):
        self.tree.close()


LAUNCHES = [(whole, mb) for whole in (True, False) for mb in (0, 3)]
LAUNCH_IDS = [f"{'tree' if w else 'buckets'}-max_blocks_{mb}" for w, mb in LAUNCHES]


# ---- 1: the encoders -------------------------------------------------------------------------
@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("launch", LAUNCHES, ids=LAUNCH_IDS)
def test_gather_q8_matches_the_checker(launch, misaligned):
    whole, mb = launch
    rig = _Rig(misaligned, mb)
    rig.feed(_grads(5))
    rig.encode(False, whole, "plain")
    # byte for byte what dl_delta_q8 writes for outer = g, inner = +0: the oracle's definition
    want = np.concatenate([oracle.delta_q8_from(h.numpy()) for h in rig.h_grads])
    assert rig.slots.cpu().numpy().tobytes() == want.tobytes()
    assert not rig.resid.cpu().numpy()[~rig.pad].any()  # no residual without error feedback
    rig.close()


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("launch", LAUNCHES, ids=LAUNCH_IDS)
def test_gather_q8_ef_matches_the_checker_over_three_steps(launch, misaligned):
    """The residual of one step feeds the next."""
    whole, mb = launch
    rig = _Rig(misaligned, mb)
    for s in (1, 2, 3):
        rig.feed(_grads(10 + s))
        rig.encode(True, whole, s)
        r = rig.resid.cpu().numpy()[~rig.pad]
        assert np.isfinite(r).all() and r.any()
    rig.close()


def test_zero_residual_gives_the_plain_encoders_slots():
    rig = _Rig()
    rig.feed(_grads(7))
    rig.encode(True, True, "ef")
    ef_slots = rig.slots.clone()
    K.gather_q8(rig.tree, ALL, SLOT_GRAD, rig.slots)
    assert torch.equal(rig.slots, ef_slots)
    rig.close()


# ---- 2: the decoder --------------------------------------------------------------------------
PART_SENTINEL = -7.0


@pytest.fixture(scope="module")
def averaged():
    """Slots as an exchange leaves them (the oracle's encoder, then its reduce over two peers),
    their decoded values per tensor and the restated partial sums; never modified."""
    a, b = _grads(21), _grads(22)
    recv = np.concatenate([np.concatenate([oracle.delta_q8_from(t) for t in g]) for g in (a, b)])
    m = recv.size // (2 * SLOT)
    slots = oracle.q8_reduce(recv, 2, m, 2)
    vals, c = [], 0
    for n in NUMELS:
        k = len(oracle.chunks_of(n))
        vals.append(oracle.q8_deq(slots[c * SLOT:(c + k) * SLOT], n))
        c += k
    assert c == m
    return dict(slots=slots, vals=vals, parts=cr.tree_partials(vals))


def _check_decoded(rig, vals, what):
    got = rig.base.cpu().numpy()
    for a, n, v in zip(rig.at, NUMELS, vals):
        assert ef.same_bits(got[a:a + n], v), (what, "dst", n)
    assert (got[rig.guard] == F(-123.25)).all(), (what, "guard floats")


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("launch", LAUNCHES, ids=LAUNCH_IDS)
def test_unpack_avg_q8_matches_the_oracle(averaged, launch, misaligned):
    whole, mb = launch
    rig = _Rig(misaligned, mb)
    slots = torch.from_numpy(averaged["slots"]).to(DEV)
    rig.h_slots.copy_(torch.from_numpy(averaged["slots"]))
    nch = rig.tree.n_chunks
    partials = torch.full((nch,), PART_SENTINEL, dtype=torch.float64, device=DEV)
    if whole:
        K.unpack_avg_q8(rig.tree, ALL, slots, SLOT_GRAD, partials)
    else:
        for b in reversed(range(rig.tree.n_buckets)):
            K.unpack_avg_q8(rig.tree, b, rig.bucket_slots(slots, b), SLOT_GRAD, partials)
            c0, c1 = rig.tree.bucket_chunks[b]
            p = partials.cpu().numpy()
            # a bucket launch writes exactly its chunk range
            assert (p[:c0] == PART_SENTINEL).all() and (p[c0:c1] != PART_SENTINEL).all(), b
    torch.cuda.synchronize()
    _check_decoded(rig, averaged["vals"], "partials")
    assert slots.cpu().numpy().tobytes() == averaged["slots"].tobytes()  # only read
    # the checker backend, the restatement, and dl_grad_sumsq on the destination afterwards
    h_part = torch.full((nch,), PART_SENTINEL, dtype=torch.float64)
    REF.unpack_avg_q8(rig.cpu, ALL, rig.h_slots, SLOT_GRAD, h_part)
    for h, v in zip(rig.h_grads, averaged["vals"]):
        assert h.numpy().tobytes() == v.tobytes()
    got = partials.cpu().numpy()
    assert got.tobytes() == h_part.numpy().tobytes()
    assert got.tobytes() == averaged["parts"].tobytes()
    again = torch.full((nch,), PART_SENTINEL, dtype=torch.float64, device=DEV)
    K.grad_sumsq(rig.tree, ALL, SLOT_GRAD, again)
    assert again.cpu().numpy().tobytes() == got.tobytes()
    rig.close()


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
def test_unpack_avg_q8_without_partials(averaged, misaligned):
    rig = _Rig(misaligned)
    slots = torch.from_numpy(averaged["slots"]).to(DEV)
    for b in range(rig.tree.n_buckets):
        K.unpack_avg_q8(rig.tree, b, rig.bucket_slots(slots, b), SLOT_GRAD)
    torch.cuda.synchronize()
    _check_decoded(rig, averaged["vals"], "no partials")
    rig.base.fill_(-123.25)
    K.unpack_avg_q8(rig.tree, ALL, slots, SLOT_GRAD, None)
    torch.cuda.synchronize()
    _check_decoded(rig, averaged["vals"], "no partials, whole tree")
    rig.close()


# ---- 3: special values -----------------------------------------------------------------------
@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("feedback", [False, True], ids=["plain", "ef"])
def test_special_values(feedback, misaligned):
    """An all-zero chunk (scale 0, every q 0), a chunk with one NaN (fmaxf ignores it: a finite
    scale), one with +Inf (s = Inf: 0 · Inf decodes to NaN), and a chunk of denormals (kept: s
    itself is subnormal): slots, residual, decoded values and partials against the checker."""
    rng = np.random.default_rng(31)
    grads = [(rng.standard_normal(n) * 0.02).astype(F) for n in NUMELS]
    resid = [(rng.standard_normal(n) * 1e-4).astype(F) for n in NUMELS]
    grads[3][:], resid[3][:] = 0.0, 0.0  # 4095: all zero
    grads[4][1234] = np.nan  # 4096: one NaN
    grads[5][17] = np.inf  # first chunk of 4097
    grads[2][:] = (rng.standard_normal(257) * 1e-40).astype(F)  # denormals only
    resid[2][:] = (rng.standard_normal(257) * 1e-41).astype(F)
    grads[6][8197 - 2] = np.nan  # the tail of the last chunk
    rig = _Rig(misaligned)
    rig.feed(grads, resid if feedback else None)
    rig.encode(feedback, False, "special")
    s = rig.h_slots.numpy()
    scale = lambda c: s[c * SLOT:c * SLOT + 4].view(F)[0]  # noqa: E731
    assert scale(3) == 0 and np.isfinite(scale(4)) and scale(4) > 0 and np.isinf(scale(5))
    assert 0 < scale(2) < np.finfo(F).tiny
    nch = rig.tree.n_chunks
    partials = torch.full((nch,), PART_SENTINEL, dtype=torch.float64, device=DEV)
    h_part = torch.zeros(nch, dtype=torch.float64)
    K.unpack_avg_q8(rig.tree, ALL, rig.slots, SLOT_GRAD, partials)
    REF.unpack_avg_q8(rig.cpu, ALL, rig.h_slots, SLOT_GRAD, h_part)
    torch.cuda.synchronize()
    _check_decoded(rig, [h.numpy() for h in rig.h_grads], "special")
    assert ef.same_bits(partials.cpu().numpy(), h_part.numpy())
    assert np.isnan(rig.h_grads[5].numpy()[:4096]).any() and not rig.h_grads[3].numpy().any()
    rig.close()


def test_argument_errors_are_raised_before_any_launch():
    tree = PackedTree([10, 20])
    s = _stream()
    buf = torch.zeros(2 * SLOT, device=DEV)
    a = buf.data_ptr()
    for name, args in (("dl_gather_q8", (a,)), ("dl_gather_q8_ef", (a, a)),
                       ("dl_unpack_avg_q8", (a, SLOT_GRAD, a))):
        head = (tree.handle, ALL) if name == "dl_unpack_avg_q8" else (tree.handle, ALL, SLOT_GRAD)
        with pytest.raises(_lib.DilocoHipError, match="not bound") as e:
            _lib.call(name, *head, *args, s)
        assert e.value.code == -2 and name in str(e.value)  # DL_E_STATE
    tree.bind(SLOT_GRAD, [torch.zeros(10, device=DEV), torch.zeros(20, device=DEV)], s)
    for name, args, msg in [
            ("dl_gather_q8", (tree.handle, ALL, SLOT_GRAD, None), "slots is null"),
            ("dl_gather_q8", (tree.handle, ALL, SLOT_GRAD, a + 8), "slots not 16-B"),
            ("dl_gather_q8", (tree.handle, 5, SLOT_GRAD, a), "bucket 5"),
            ("dl_gather_q8_ef", (tree.handle, ALL, SLOT_GRAD, None, a), "residual is null"),
            ("dl_gather_q8_ef", (tree.handle, ALL, SLOT_GRAD, a + 4, a), "residual not 16-B"),
            ("dl_gather_q8_ef", (tree.handle, ALL, SLOT_GRAD, a, None), "slots is null"),
            ("dl_unpack_avg_q8", (tree.handle, ALL, None, SLOT_GRAD, None), "slots is null"),
            ("dl_unpack_avg_q8", (tree.handle, ALL, a + 8, SLOT_GRAD, None), "slots not 16-B"),
            ("dl_unpack_avg_q8", (tree.handle, ALL, a, SLOT_GRAD, a + 4), "partials not 8-B"),
            ("dl_unpack_avg_q8", (tree.handle, ALL, a, 99, None), "slot 99")]:
        with pytest.raises(_lib.DilocoHipError, match=msg):
            _lib.call(name, *args, s)
    torch.cuda.synchronize()
    assert not buf.any()  # nothing was launched
    tree.close()


# ---- 4: GradSync, one replica ----------------------------------------------------------------
def _params(grads):
    ps = []
    for g in grads:
        p = torch.nn.Parameter(torch.zeros(g.size, device=DEV))
        p.grad = torch.from_numpy(g).to(DEV)  # a fresh tensor every step
        ps.append(p)
    return ps


def _set_grads(ps, grads):
    for p, g in zip(ps, grads):
        p.grad = torch.from_numpy(g).to(DEV)


@pytest.mark.parametrize("feedback", [False, True], ids=["plain", "ef"])
def test_gradsync_one_replica_matches_the_restatement(feedback):
    """encode -> the plain in-place re-quantise -> decode, three steps, against
    EFExchange(n=1, reduce_ef=False) (with zero residuals kept zero: the plain codec)."""
    ps = _params(_grads(40))
    gs = GradSync(ps, None, 1, wire_dtype=torch.int8, bucket_cap_elems=CAP,
                  error_feedback=feedback)
    # gs.local unless an earlier test left a one-rank process group behind: then the same three
    # kernels run around that group's collectives of one, and the bytes are the same
    assert gs.world_size == 1 and gs.tree.n_buckets >= 2
    counts = [c1 - c0 for c0, c1 in gs.tree.bucket_chunks]
    ex = ef.EFExchange(NUMELS, counts, 1, reduce_ef=False)
    for s in (1, 2, 3):
        g = _grads(40 + s)
        _set_grads(ps, g)
        assert gs.sync() is None
        torch.cuda.synchronize()
        if feedback:
            want = ex.average([g])
        else:
            want = oracle.q8_average([g], NUMELS, counts)
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
def test_gradsync_int8_with_max_norm_equals_sync_then_clip(factor):
    g = _grads(50)
    pa, pb = _params(g), _params(g)
    kw = dict(wire_dtype=torch.int8, bucket_cap_elems=CAP, error_feedback=True)
    ga, gb = GradSync(pa, None, 1, **kw), GradSync(pb, None, 1, **kw)
    for s in (1, 2):
        g = _grads(50 + s)
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


# ---- 5: two gloo ranks on the one GPU --------------------------------------------------------
STEPS = 3
NUMELS_DP = NUMELS + [5]  # 11 chunks in DPSync's one bucket: a padding slot at two peers


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out):
    for p in (PKG, REPO, os.path.join(REPO, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["DILOCO_COLLECTIVE_READ_TIMEOUT"] = "10"
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank,
                            world_size=world)
    from diloco_amd import comm
    from diloco_amd.world import World

    # the knobs come from the environment the test set before the spawn
    assert comm.DP_WIRE == "int8" and comm.DP_Q8_EF is True and comm.dp_backend() == "gloo"
    rec = {}
    for feedback in (True, False):
        comm.DP_Q8_EF = feedback
        model = torch.nn.Module()
        model.ps = torch.nn.ParameterList(
            [torch.nn.Parameter(torch.zeros(n, device=DEV)) for n in NUMELS_DP])
        dp = comm.DPSync(World.from_default_group(1))
        ex = None
        for s in range(1, STEPS + 1):
            by_rank = [_grads(100 * s + r, NUMELS_DP) for r in range(world)]
            for p, g in zip(model.parameters(), by_rank[rank]):
                p.grad = torch.from_numpy(g).to(DEV)  # reallocated every step
            assert dp.sync_gradients(model) is None
            torch.cuda.synchronize()
            if ex is None:
                gs = next(iter(dp._grad_syncs.values()))
                assert gs.q8 and gs.error_feedback == feedback and not gs.local
                counts = [c1 - c0 for c0, c1 in gs.tree.bucket_chunks]
                rec["counts"] = np.array(counts)
                ex = ef.EFExchange(NUMELS_DP, counts, world)
            want = ex.average(by_rank) if feedback else oracle.q8_average(
                by_rank, NUMELS_DP, counts)
            tag = f"{'ef' if feedback else 'plain'}_s{s}"
            rec["grad_" + tag] = np.concatenate(
                [p.grad.cpu().numpy() for p in model.parameters()])
            rec["ref_" + tag] = np.concatenate(want)
        if feedback:
            st = gs.q8_ef_state()
            rec["encode_nonzero"] = np.array(bool(st["encode"].any()))
            rec["reduce"] = np.concatenate([a.cpu().numpy() for a in st["reduce"]])
            rec["ref_reduce"] = np.concatenate([ex.red[b][rank] for b in range(len(ex.red))])
    np.savez(os.path.join(out, f"r{rank}.npz"), **rec)
    dist.barrier()
    dist.destroy_process_group()


def test_dpsync_int8_wire_two_peers_on_gpu(monkeypatch):
    """Two gloo processes on the one GPU, DPSync.sync_gradients under DILOCO_DP_WIRE=int8 with
    error feedback on and off, three steps each: dl_gather_q8[_ef] -> all_to_all ->
    dl_q8_reduce[_ef] -> all_gather -> dl_unpack_avg_q8. Both ranks end with the same bytes,
    equal to the exchange composed by hand."""
    monkeypatch.setenv("DILOCO_DP_BACKEND", "gloo")
    monkeypatch.setenv("DILOCO_DP_WIRE", "int8")
    monkeypatch.setenv("DILOCO_DP_Q8_EF", "1")
    monkeypatch.delenv("DILOCO_DP_EXCHANGE", raising=False)
    out = tempfile.mkdtemp(prefix="dl_gradsync_q8_")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    recs = [dict(np.load(os.path.join(out, f"r{r}.npz"))) for r in range(2)]
    assert any(int(c) % 2 for c in recs[0]["counts"])
    for rec in recs:
        for mode in ("ef", "plain"):
            for s in range(1, STEPS + 1):
                got, want = rec[f"grad_{mode}_s{s}"], rec[f"ref_{mode}_s{s}"]
                assert got.tobytes() == want.tobytes(), (mode, s, int((got != want).sum()))
                assert got.tobytes() == recs[0][f"grad_{mode}_s{s}"].tobytes(), (mode, s)
        assert bool(rec["encode_nonzero"])
        assert rec["reduce"].tobytes() == rec["ref_reduce"].tobytes() and rec["reduce"].any()
