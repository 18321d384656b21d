"""The 4-bit (MXFP4) wire on the GPU: dl_delta_fp4, dl_fp4_reduce, dl_unpack_sgd_fp4 and
dl_unpack_adamw_fp4 against the numpy restatement (tests/fp4_restatement.py, walked over the
packed layout by tests/fp4_oracle_kernels.py), bit for bit, NaNs by position; nothing is skipped
or masked.

The tree is small and adversarial: a 1-element chunk, 31 and 33 elements (one short of and one
past a group of 32), a chunk one short of full, a full one, tensors that spill 1 and 3 elements
into a second chunk, a three-chunk tensor with a tail that is no multiple of 4, and a four-chunk
one whose tail is no multiple of 32. Bucket cap 8192 splits it into several buckets. Inner
tensors sit in their own allocations (16-B aligned: a group is 8 lanes of a float4 row) or one
float off (the element-wise path: a group is 32 lanes)."""
import os
import socket
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import fp4_footprint as f4
import fp4_restatement as fp4
from conftest import PKG, REPO
from diloco_amd import _lib, synth
from diloco_amd.kernels import HipKernels, adamw_scalars, set_default_kernels
from diloco_amd.plan import SLOT_INNER, PackedTree
from diloco_amd.trees import get_tree
from fp4_oracle_kernels import Fp4OracleKernels
from oracle import oracle
from oracle_kernels import CpuTree

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
NUMELS = [1, 31, 33, 4095, 4096, 4097, 4099, 8217, 14338]
CAP = 8192
SLOT, CHUNK = fp4.SLOT, fp4.CHUNK
ALL = _lib.ALL_BUCKETS
SENTINEL = 0x7F8BEEF5  # a NaN bit pattern: the padding of the packed arenas before every run
K = HipKernels()
REF = Fp4OracleKernels()


def _pseudo_gradient_tree(rng):
    """θ and inner whose difference spreads over five decades inside every group of 32, so every
    code and many scales occur and most elements leave a residual."""
    theta = [rng.standard_normal(n).astype(F) for n in NUMELS]
    inner = []
    for t in theta:
        d = (10.0 ** rng.uniform(-5, 0, t.size) * rng.choice([-1.0, 1.0], t.size)).astype(F)
        inner.append((t - d).astype(F))
    return theta, inner


class _Rig:
    """One tree on the device (θ, residual, slots, inner tensors) and its host twin on the
    checker backend, fed the same values. The residual's padding holds a sentinel."""

    def __init__(self, misaligned=False, max_blocks=0):
        self.tree = PackedTree(NUMELS, CAP)
        self.cpu = CpuTree(NUMELS, CAP)
        assert self.tree.n_buckets >= 3 and self.tree.bucket_chunks == self.cpu.bucket_chunks
        assert self.tree.total == self.cpu.total
        if max_blocks:
            self.tree.tune(max_blocks)
        self.offs = [int(o) for o in self.tree.seg_off[:-1]]
        self.pad = np.ones(self.tree.total, dtype=bool)
        for o, n in zip(self.offs, NUMELS):
            self.pad[o:o + n] = False
        z = dict(dtype=torch.float32, device=DEV)
        res0 = np.zeros(self.tree.total, dtype=np.uint32)
        res0[self.pad] = SENTINEL
        self.res0 = res0.view(F).copy()
        self.theta = torch.zeros(self.tree.total, **z)
        self.resid = torch.from_numpy(self.res0.copy()).to(DEV)
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
        self.h_resid = torch.from_numpy(self.res0.copy())
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

    def encode(self, ef, whole=False, reference=True):
        res = self.resid if ef else None
        self.slots.fill_(0xEE)  # every byte of every launched slot is written
        if whole:
            K.delta_fp4(self.tree, ALL, SLOT_INNER, self.theta, res, self.slots)
        else:
            for b in range(self.tree.n_buckets):
                K.delta_fp4(self.tree, b, SLOT_INNER, self.theta, res,
                            self.bucket_slots(self.slots, b))
        if reference:
            REF.delta_fp4(self.cpu, ALL, SLOT_INNER, self.h_theta, self.h_resid if ef else None,
                          self.h_slots)
        torch.cuda.synchronize()

    def check(self, what, ef):
        got_s, want_s = self.slots.cpu().numpy(), self.h_slots.numpy()
        assert got_s.tobytes() == want_s.tobytes(), (what, "slots", int((got_s != want_s).sum()))
        pay = got_s.reshape(-1, SLOT)[:, fp4.N_GROUPS:]
        assert not ((pay & 15) == 8).any() and not ((pay >> 4) == 8).any(), (what, "nibble 8")
        got_r, want_r = self.resid.cpu().numpy(), self.h_resid.numpy()
        if ef:
            assert fp4.same_bits(got_r[~self.pad], want_r[~self.pad]), (what, "residual")
        else:  # the plain encoder never touches a residual
            assert got_r.tobytes() == self.res0.tobytes(), (what, "residual untouched")
        assert (got_r.view(np.uint32)[self.pad] == SENTINEL).all(), (what, "padding")


@pytest.mark.parametrize("ef", [False, True])
@pytest.mark.parametrize("misaligned", [False, True])
def test_delta_fp4_matches_the_restatement(misaligned, ef):
    """Three consecutive steps, bucket by bucket: the residual of one step feeds the next."""
    rng = np.random.default_rng(61)
    rig = _Rig(misaligned)
    for s in (1, 2, 3):
        rig.feed(*_pseudo_gradient_tree(rng))
        rig.encode(ef)
        rig.check(s, ef)
        if ef:
            r = rig.resid.cpu().numpy()[~rig.pad]
            assert np.isfinite(r).all() and r.any()
    rig.tree.close()


@pytest.mark.parametrize("ef", [False, True])
def test_delta_fp4_does_not_depend_on_the_launch_shape_or_alignment(ef):
    """Per bucket, one whole-tree launch, and two workgroups walking all the chunks (the LDS
    stage is reused chunk after chunk), on 16-B-aligned and on 4-B-aligned inner tensors: the
    same bytes, two steps."""
    rng = np.random.default_rng(67)
    rigs = [_Rig(m, max_blocks=g) for m in (False, True) for g in (0, 0, 2)]
    for s in (1, 2):
        theta, inner = _pseudo_gradient_tree(rng)
        for i, rig in enumerate(rigs):
            rig.feed(theta, inner)
            rig.encode(ef, whole=i % 3 > 0, reference=i == 0)
        rigs[0].check(s, ef)
        for rig in rigs[1:]:
            assert torch.equal(rig.slots, rigs[0].slots), s
            assert torch.equal(rig.resid.view(torch.int32), rigs[0].resid.view(torch.int32)), s
    for rig in rigs:
        rig.tree.close()


def test_zero_residual_gives_the_plain_encoders_slots():
    rng = np.random.default_rng(71)
    rig = _Rig()
    rig.feed(*_pseudo_gradient_tree(rng), resid=[np.zeros(n, dtype=F) for n in NUMELS])
    rig.encode(False, whole=True, reference=False)
    plain = rig.slots.clone()
    rig.encode(True, whole=True, reference=False)
    assert torch.equal(rig.slots, plain)
    rig.tree.close()


MAXF = float(np.finfo(F).max)
TWO = lambda k: float(np.ldexp(1.0, k))  # noqa: E731
# (θ, inner, residual) triples: NaN, ±Inf, ±FLT_MAX whose difference overflows
WILD = [(np.nan, 1.0, 0.0), (np.inf, 1.0, 0.0), (-np.inf, np.inf, 0.0), (1.0, 1.0, np.inf),
        (MAXF, -MAXF, 0.0), (-MAXF, MAXF, 1.0), (1.0, 0.0, np.nan), (0.0, 0.0, -np.inf)]
# finite oddities: signed zeros, denormals, values that clamp the scale to E = 0 and E = 1
TAME = [(0.0, -0.0, 0.0), (-0.0, 0.0, -0.0), (-0.0, -0.0, -0.0), (1e-40, 2e-40, 0.0),
        (0.0, 0.0, 1e-40), (5e-39, -5e-39, -3e-41), (1e-38, 1.1e-38, 1e-45), (TWO(-128), 0.0, 0.0),
        (0.0, TWO(-127), 0.0), (TWO(-126), 0.0, TWO(-149))]
TIES = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]


@pytest.mark.parametrize("ef", [False, True])
@pytest.mark.parametrize("misaligned", [False, True])
def test_delta_fp4_special_values(misaligned, ef):
    """One step. Every non-finite x turns its own group of 32 into E = 255 (decoded NaN, NaN
    residuals) and no other; groups of ±0 and denormals stay finite at E = 0; a group at
    E = 253; the tie table at scale 1, both signs."""
    rng = np.random.default_rng(73)
    theta = [(rng.standard_normal(n) * 0.02).astype(F) for n in NUMELS]
    inner = [(rng.standard_normal(n) * 0.02).astype(F) for n in NUMELS]
    resid = [(rng.standard_normal(n) * 1e-4).astype(F) for n in NUMELS]

    def plant(t, at, triples):
        for k, (a, b, c) in enumerate(triples):
            theta[t][at + k], inner[t][at + k], resid[t][at + k] = a, b, c if ef else 0.0

    for k, w in enumerate(WILD):  # one per group of the full chunk: groups 0, 2, 4, ...
        plant(4, 64 * k + k, [w])
    plant(7, 4096 - 2, WILD[:4])  # across a chunk boundary: the last and the first group
    plant(7, 8217 - 1, [(np.nan, 0.0, 0.0)])  # the last element of a tail no multiple of 4
    plant(8, 14338 - 2, [(1.0, np.nan, 0.0)])  # a tail no multiple of 32
    for t in (2, 3):  # finite oddities only, in tensors that hold nothing else
        theta[t][:], inner[t][:], resid[t][:] = 0.0, 0.0, 0.0
    plant(2, 33 - len(TAME), TAME)
    plant(3, 0, TAME)
    plant(3, 32, [(6.0, 0.0, 0.0)] + [(0.0, -v, 0.0) for v in TIES] + [(-v, 0.0, 0.0) for v in TIES])
    plant(3, 64, [(3.25 * TWO(126), 0.0, 0.0), (0.0, TWO(126), 0.0), (TWO(125), 0.0, 0.0)])
    plant(3, 96, [(6 * TWO(-126), 0.0, 0.0), (0.0, TWO(-126), 0.0), (TWO(-127), 0.0, 0.0)])
    rig = _Rig(misaligned)
    rig.feed(theta, inner, resid if ef else None)
    rig.encode(ef)
    rig.check("special", ef)
    slots = rig.slots.cpu().numpy()
    c4 = [c for c, ch in enumerate(rig.cpu.chunks) if ch[0] == 4][0]
    e4 = slots[c4 * SLOT:c4 * SLOT + fp4.N_GROUPS]
    with np.errstate(all="ignore"):  # which triples give a non-finite x, from the inputs alone
        bad = [k for k, (a, b, c) in enumerate(WILD)
               if not np.isfinite(F(F(a) - F(b)) + (F(c) if ef else F(0)))]
    assert len(bad) == (len(WILD) if ef else 5)
    assert sorted(np.nonzero(e4 == 255)[0].tolist()) == [2 * k for k in bad]
    c3 = [c for c, ch in enumerate(rig.cpu.chunks) if ch[0] == 3][0]
    s3 = slots[c3 * SLOT:(c3 + 1) * SLOT]
    assert s3[:4].tolist() == [0, 127, 253, 1]
    deq = fp4.decode_slot(s3, 4095)
    assert deq[33:47].tolist() == [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0] + \
        [-0.0, -1.0, -1.0, -2.0, -2.0, -4.0, -4.0]
    assert np.isfinite(deq).all() and deq[7] == F(TWO(-128)) and deq[8] == F(-TWO(-127))
    if ef:
        r = rig.resid.cpu().numpy()
        got = [r[o:o + n] for o, n in zip(rig.offs, NUMELS)]
        assert np.isfinite(got[2]).all() and np.isfinite(got[3]).all()
        nan4 = np.isnan(got[4]).reshape(-1, 32)
        assert nan4[[2 * k for k in bad]].all() and nan4.sum() == 32 * len(bad)
        assert np.isnan(got[7][8192:8217]).all() and not np.isnan(got[7][4128:8192]).any()
        assert np.isnan(got[8][14336:]).all() and not np.isnan(got[8][:14336]).any()
    rig.tree.close()


def test_fp4_argument_errors_are_raised():
    tree = PackedTree([10, 20])
    s = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(2 * SLOT, device=DEV)
    a = buf.data_ptr()
    with pytest.raises(_lib.DilocoHipError, match="not bound") as e:
        _lib.call("dl_delta_fp4", tree.handle, ALL, SLOT_INNER, a, a, a, s)
    assert e.value.code == -2 and "dl_delta_fp4" in str(e.value)  # DL_E_STATE
    tree.bind(SLOT_INNER, [torch.zeros(10, device=DEV), torch.zeros(20, device=DEV)], s)
    for args, msg in [((a, a + 4, a), "residual not 16-B"), ((None, a, a), "outer is null"),
                      ((a, a, None), "slots is null"), ((a, None, a + 8), "slots not 16-B")]:
        with pytest.raises(_lib.DilocoHipError, match=msg) as e:
            _lib.call("dl_delta_fp4", tree.handle, ALL, SLOT_INNER, *args, s)
        assert e.value.code == (-1 if "null" in msg else -3)  # DL_E_ARG / DL_E_ALIGN
    with pytest.raises(_lib.DilocoHipError, match="slots is null"):
        _lib.call("dl_unpack_sgd_fp4", tree.handle, ALL, None, a, a, 0.7, 0.9, 1, 0, -1, s)
    with pytest.raises(_lib.DilocoHipError, match="exp_avg_sq not 16-B"):
        _lib.call("dl_unpack_adamw_fp4", tree.handle, ALL, a, a, a, a + 4, 1.0, 0.1, 0.95, 0.05,
                  -0.1, 1.0, 1e-8, -1, s)
    torch.cuda.synchronize()
    assert not buf.any()  # nothing was launched
    tree.close()


# ---- the reduce ------------------------------------------------------------------------------
M = 5  # slots per peer: a multiple of neither 2 nor 3


def _peer_slots(rng, n_peers):
    """n_peers x M slots: full chunks, a short one (zero tail), one with a NaN group, and an
    all-zero padding slot last."""
    recv = np.zeros(n_peers * M * SLOT, dtype=np.uint8)
    for r in range(n_peers):
        for j, n in enumerate((CHUNK, 1000, CHUNK, 33)):
            x = (10.0 ** rng.uniform(-4, 0, n) * rng.choice([-1.0, 1.0], n)).astype(F)
            if j == 2 and r == n_peers - 1:
                x[77] = np.nan
            at = (r * M + j) * SLOT
            recv[at:at + SLOT] = fp4.encode_values(x)
    return recv


@pytest.mark.parametrize("ef", [False, True])
@pytest.mark.parametrize("n_peers, divisor", [(1, 1), (2, 2), (2, 1), (3, 3), (3, 1)])
def test_fp4_reduce_matches_the_restatement(n_peers, divisor, ef):
    """Two steps from a residual that is already nonzero where the slots hold values; at one
    peer in place. Every byte of the output slots is written (they hold garbage before)."""
    rng = np.random.default_rng(79 + n_peers)
    res = None
    if ef:
        res = np.zeros(M * CHUNK, dtype=F)
        res[:CHUNK + 1000] = (1e-3 * rng.standard_normal(CHUNK + 1000)).astype(F)
        d_res = torch.from_numpy(res).to(DEV)
    for s in (1, 2):
        recv = _peer_slots(rng, n_peers)
        want, res = fp4.reduce_slots(recv, n_peers, M, divisor, res)
        d_recv = torch.from_numpy(recv).to(DEV)
        d_out = d_recv if n_peers == 1 else torch.full((M * SLOT,), 0xEE, dtype=torch.uint8,
                                                       device=DEV)
        K.fp4_reduce(d_recv, n_peers, M, divisor, d_res if ef else None, d_out)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert got.tobytes() == want.tobytes(), (s, int((got != want).sum()))
        assert not want[4 * SLOT:].any()  # the padding slot stays all zero
        assert (want[2 * SLOT:2 * SLOT + fp4.N_GROUPS] == 255).sum() == 1  # the NaN group, alone
        if n_peers > 1:
            assert d_recv.cpu().numpy().tobytes() == recv.tobytes()  # the input is only read
        if ef:
            assert fp4.same_bits(d_res.cpu().numpy(), res), s
            assert not res[4 * CHUNK:].any() and res[:CHUNK].any()
        elif n_peers == 1:
            # the identity on decoded values (the bytes may differ: a group whose largest
            # element rounded down re-encodes at a finer scale, to the same values)
            for j in range(M):
                assert fp4.same_bits(fp4.decode_slot(got[j * SLOT:(j + 1) * SLOT]),
                                     fp4.decode_slot(recv[j * SLOT:(j + 1) * SLOT])), (s, j)


# ---- the fused steps -------------------------------------------------------------------------
LR, MOMENTUM = 0.7, 0.9
ADAM = [adamw_scalars(0.01, 0.9, 0.95, 0.1, 1e-8, t) for t in (1, 2)]


def _packed(rng, rig, fill):
    x = rig.res0.copy()
    for o, n in zip(rig.offs, NUMELS):
        v = rng.standard_normal(n).astype(F)
        x[o:o + n] = v * v * F(0.01) if fill == "square" else v
    return torch.from_numpy(x).to(DEV)


def _decoded_wire(rig):
    """The rig's slots decoded on the host into an fp32 wire (the packed layout)."""
    slots = rig.slots.cpu().numpy()
    wire = rig.res0.copy()
    for c, (_seg, _o, n, po) in enumerate(rig.cpu.chunks):
        wire[po:po + n] = fp4.decode_slot(slots[c * SLOT:(c + 1) * SLOT], n)
    return torch.from_numpy(wire).to(DEV)


def _same(a, b, pad, what):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert a.view(np.uint32)[pad].tolist() == b.view(np.uint32)[pad].tolist() == \
        [SENTINEL] * int(pad.sum()), (what, "padding")
    assert fp4.same_bits(a[~pad], b[~pad]), what


def _fused_rigs(misaligned, rng):
    """Two rigs fed alike: one steps from the slots, one from the decoded fp32 wire."""
    a, b = _Rig(misaligned), _Rig(misaligned)
    theta, inner = _pseudo_gradient_tree(rng)
    inner[4][100] = np.nan  # one NaN group: NaNs are compared by position
    for rig in (a, b):
        rig.feed(theta, inner)
        pad = torch.from_numpy(rig.pad).to(DEV)
        rig.theta[pad] = torch.from_numpy(rig.res0).to(DEV)[pad]  # θ's padding: the sentinel
    a.encode(False, reference=False)
    b.slots.copy_(a.slots)
    return a, b, _decoded_wire(a)


@pytest.mark.parametrize("write_inner", [True, False])
@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("momentum, nesterov", [(0.0, False), (MOMENTUM, True), (MOMENTUM, False)])
def test_unpack_sgd_fp4_equals_decode_then_unpack_sgd(momentum, nesterov, misaligned, write_inner):
    """The first step (MODE 1, or MODE 0 without momentum) and the steady one (MODE 2), bucket by
    bucket against one whole-tree launch of dl_unpack_sgd on the decoded wire."""
    rng = np.random.default_rng(89)
    a, b, wire = _fused_rigs(misaligned, rng)
    ma, mb = (_packed(rng, a, "normal") for _ in range(2)) if momentum else (None, None)
    if momentum:
        mb.copy_(ma)
    slot = SLOT_INNER if write_inner else -1
    for first in (True, False):
        before = [t.clone() for t in a.inner]
        for k in range(a.tree.n_buckets):
            K.unpack_sgd_fp4(a.tree, k, a.bucket_slots(a.slots, k), a.theta, ma, LR, momentum,
                             nesterov, first, slot)
        K.unpack_sgd(b.tree, ALL, wire, 1, b.theta, mb, LR, momentum, nesterov, first, slot)
        torch.cuda.synchronize()
        _same(a.theta, b.theta, a.pad, ("theta", first))
        if momentum:
            _same(ma, mb, a.pad, ("momentum", first))
        for t, (x, y, z) in enumerate(zip(a.inner, b.inner, before)):
            assert fp4.same_bits(x.cpu().numpy(), y.cpu().numpy()), ("inner", first, t)
            if not write_inner:
                assert fp4.same_bits(x.cpu().numpy(), z.cpu().numpy()), ("inner kept", first, t)
    assert np.isnan(a.theta.cpu().numpy()[~a.pad]).sum() == 32
    for rig in (a, b):
        rig.tree.close()


@pytest.mark.parametrize("write_inner", [True, False])
@pytest.mark.parametrize("misaligned", [False, True])
def test_unpack_adamw_fp4_equals_decode_then_unpack_adamw(misaligned, write_inner):
    rng = np.random.default_rng(97)
    a, b, wire = _fused_rigs(misaligned, rng)
    m1a, m2a = _packed(rng, a, "normal"), _packed(rng, a, "square")
    m1b, m2b = m1a.clone(), m2a.clone()
    slot = SLOT_INNER if write_inner else -1
    for t in (0, 1):
        K.unpack_adamw_fp4(a.tree, ALL, a.slots, a.theta, m1a, m2a, ADAM[t], slot)
        for k in range(b.tree.n_buckets):
            K.unpack_adamw(b.tree, k, wire, 1, b.theta, m1b, m2b, ADAM[t], slot)
        torch.cuda.synchronize()
        _same(a.theta, b.theta, a.pad, ("theta", t))
        _same(m1a, m1b, a.pad, ("exp_avg", t))
        _same(m2a, m2b, a.pad, ("exp_avg_sq", t))
        for i, (x, y) in enumerate(zip(a.inner, b.inner)):
            assert fp4.same_bits(x.cpu().numpy(), y.cpu().numpy()), ("inner", t, i)
    assert np.isnan(a.theta.cpu().numpy()[~a.pad]).sum() == 32
    for rig in (a, b):
        rig.tree.close()


# ---- write footprints (tests/footprint.py's arena, sentinels and comparison) -----------------
@pytest.mark.parametrize("row", list(f4.TREE_ROWS))
def test_tree_walker_footprint(row):
    """Both sentinels, inner tensors 0, 1 and mixed 0-3 elements off a 16-B boundary, whole-tree
    and bucket by bucket, grid caps 0, 1, 2 and 5, two consecutive launches: after every launch
    every byte of every buffer equals the CPU reference's."""
    for case in f4.TREE_ROWS[row]():
        f4.run_case(case, K, DEV, grids=f4.fpt.GRIDS)


@pytest.mark.parametrize("row", list(f4.FLAT_ROWS))
def test_reduce_footprint(row):
    for case in f4.FLAT_ROWS[row]():
        f4.run_flat_case(case, K, DEV)


# ---- the drop-in surface ---------------------------------------------------------------------
SGD = dict(lr=0.7, momentum=0.9, nesterov=True)
ADAMW = dict(lr=0.01, betas=(0.9, 0.95), weight_decay=0.1)
STEPS = 3


class _Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _flat(ts):
    return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in ts])


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, rule, out):
    for p in (PKG, REPO, os.path.join(REPO, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import expect

    os.environ["DILOCO_DP_BACKEND"] = "gloo"
    os.environ["DILOCO_OUTER_BUCKET_ELEMS"] = str(expect.MICRO_Q8_CAP)
    os.environ["DILOCO_OUTER_ADAMW"] = "fused"
    for v in ("DILOCO_OUTER_EXCHANGE", "DILOCO_DP_EXCHANGE", "DILOCO_OUTER_WIRE",
              "DILOCO_OUTER_FUSED", "DILOCO_OUTER_Q8_EF", "DILOCO_OUTER_FP4_EF"):
        os.environ.pop(v, None)
    os.environ["DILOCO_COLLECTIVE_READ_TIMEOUT"] = "10"
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank,
                            world_size=world)
    from adamw_restatement import AdamWState
    from diloco_amd.comm import TrainingComm
    from diloco_amd.utils import (compute_pseudo_gradient, get_optimizer, get_outer_model,
                                  outer_mirror, q8_error_feedback_state, sync_inner_model)
    from diloco_amd.world import World

    launches = []
    names = ("delta_fp4", "fp4_reduce", "unpack_sgd_fp4", "unpack_adamw_fp4", "delta_q8",
             "delta_q8_ef", "q8_reduce", "q8_reduce_ef")
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
        theta0 = synth.outer_tree(numels, spec.init_spec())
        inner = torch.nn.Module()
        inner.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(v.copy()).view(s))
                                           for v, s in zip(theta0, shapes)])
        outer = get_outer_model(inner, placement="device", wire="fp4", error_feedback=True)
        inner = inner.to(DEV)
        if rule == "sgd":
            opt = get_optimizer(outer, _Cfg(type="SGD", **SGD))
            theta = [t.copy() for t in theta0]
            buf = [np.empty_like(t) for t in theta]
        else:
            opt = get_optimizer(outer, _Cfg(type="AdamW", **ADAMW))
            ref = AdamWState(theta0, **ADAMW)
            theta = ref.theta
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
                dev = getattr(m, "dev", m)
                counts = [c1 - c0 for c0, c1 in dev.tree.bucket_chunks]
                rec["n_buckets"] = np.int64(dev.tree.n_buckets)
                ex = fp4.Fp4Exchange(numels, counts, world)
            deltas = [[oracle.delta(t, i) for t, i in zip(theta, v)] for v in vals]
            avg = ex.average(deltas)
            if rule == "sgd":
                for t in range(len(theta)):
                    oracle.sgd(theta[t], buf[t], avg[t], SGD["lr"], SGD["momentum"], True, s == 1)
            else:
                ref.step_grads(avg)
                theta = ref.theta
            torch.cuda.synchronize()
            rec[f"theta_s{s}"] = _flat(outer.parameters())
            rec[f"inner_s{s}"] = _flat(inner.parameters())
            rec[f"ref_theta_s{s}"] = np.concatenate(theta)
            rec[f"grad_s{s}"] = _flat([p.grad for p in outer.parameters()])  # decoded when read
            rec[f"ref_grad_s{s}"] = np.concatenate(avg)
        st = q8_error_feedback_state(outer)
        rec["encode"] = st["encode"].cpu().numpy()
        rec["ref_encode"] = np.zeros(dev.tree.total, dtype=F)
        for t, o in enumerate(dev.offs):
            rec["ref_encode"][o:o + numels[t]] = ex.enc[rank][t]
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


@pytest.mark.parametrize("rule", ["sgd", "adamw"])
def test_dropin_fp4_wire_two_peers_on_gpu(rule):
    """Two gloo processes on the one GPU, placement="device", wire="fp4", error_feedback=True,
    three outer steps: dl_delta_fp4 -> all_to_all -> dl_fp4_reduce -> all_gather ->
    dl_unpack_sgd_fp4 / dl_unpack_adamw_fp4 per bucket. θ, inner, .grad and both residuals equal
    the restatement bit for bit on both ranks (NaNs by position)."""
    out = tempfile.mkdtemp(prefix="dl_fp4_")
    mp.spawn(_worker, args=(2, _free_port(), rule, out), nprocs=2, join=True)
    recs = [dict(np.load(os.path.join(out, f"r{r}.npz"))) for r in range(2)]
    for rec in recs:
        nb = int(rec["n_buckets"])
        assert nb >= 3
        launches = [str(x) for x in rec["launches"]]
        assert launches.count("delta_fp4") == launches.count("fp4_reduce") == nb * STEPS
        assert launches.count("unpack_adamw_fp4" if rule == "adamw" else "unpack_sgd_fp4") == \
            nb * STEPS
        assert not [x for x in launches if "q8" in x]
        for s in range(1, STEPS + 1):
            got, want = rec[f"theta_s{s}"], rec[f"ref_theta_s{s}"]
            assert fp4.same_bits(got, want), (s, int((got != want).sum()))
            assert fp4.same_bits(rec[f"inner_s{s}"], want), s
            assert fp4.same_bits(rec[f"grad_s{s}"], rec[f"ref_grad_s{s}"]), s
            assert got.tobytes() == recs[0][f"theta_s{s}"].tobytes(), s
        assert fp4.same_bits(rec["encode"], rec["ref_encode"]) and rec["encode"].any()
        assert fp4.same_bits(rec["reduce"], rec["ref_reduce"]) and rec["reduce"].any()
