"""The top-k wire with 4-bit values on the GPU: dl_delta_topk_fp4, dl_topk_fp4_reduce,
dl_unpack_sgd_topk_fp4 and dl_unpack_adamw_topk_fp4 against the numpy restatement
(tests/topk_fp4_restatement.py), bit for bit, NaNs by position. The tree, the rig (sentinels in
the arenas' padding, slots pre-filled with 0xEE, inner tensors 16-B aligned or one float off) and
the two-peer worker are test_topk_gpu.py's, under this wire's slot size and kernels."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import test_topk_gpu as base
import topk_fp4_restatement as tq
from diloco_amd.mirror import _decode_topk_fp4
from diloco_amd.plan import SLOT_INNER
from test_topk_gpu import ADAM, ALL, DEV, EDGE, NUMELS, F, K, N, _decades, _put

pytestmark = pytest.mark.gpu
SB = tq.slot_bytes


class _Rig(base._Rig):
    def __init__(self, k, misaligned, numels=NUMELS):
        super().__init__(k, misaligned, numels)
        self.slots = torch.zeros(self.tree.n_chunks * SB(k), dtype=torch.uint8, device=DEV)

    def encode(self, theta, inner, resid, mode="buckets"):
        for d, i in zip(self.inner, inner):
            d.copy_(torch.from_numpy(i))
        th = self.packed(theta)
        res = self.packed(resid) if resid is not None else None
        self.slots.fill_(0xEE)
        self.tree.tune(3 if mode == "grid3" else 0)
        for b in ([ALL] if mode != "buckets" else range(self.tree.n_buckets)):
            c0 = 0 if b == ALL else self.tree.bucket_chunks[b][0]
            K.delta_topk_fp4(self.tree, b, SLOT_INNER, th, res, self.k, self.slots[c0 * SB(self.k):])
        torch.cuda.synchronize()
        return res


def _expect(theta, inner, resid, k):
    enc = [tq.encode_tensor(t - i, k, r) for t, i, r in
           zip(theta, inner, resid if resid is not None else [None] * len(theta))]
    return np.concatenate([s for s, _ in enc]), [r for _, r in enc]


def _same(got, want, what):
    assert got.cpu().numpy().tobytes() == want.tobytes(), what


@pytest.mark.parametrize("k", [8, 40, 256])  # one ragged group; a full and a ragged one; all lanes
@pytest.mark.parametrize("ef", [False, True])
@pytest.mark.parametrize("misaligned", [False, True])
def test_delta_topk_fp4_matches_the_restatement_and_fp64(misaligned, ef, k):
    rng = np.random.default_rng(k)
    rig = _Rig(k, misaligned)
    theta = [rng.standard_normal(n).astype(F) for n in NUMELS]
    inner = [(t - rng.standard_normal(t.size).astype(F)).astype(F) for t in theta]
    resid = [(rng.standard_normal(n) / 8).astype(F) for n in NUMELS] if ef else None
    want_s, want_r = _expect(theta, inner, resid, k)
    for mode in ("buckets", "whole", "grid3"):
        res = rig.encode(theta, inner, resid, mode)
        _same(rig.slots, want_s, mode)
        if ef:
            rig.check(res, want_r, (mode, "residual"))
    # against fp64, no restatement: the k largest |x| in stable order; every decoded entry within
    # 2^(E-127) of x (E2M1's widest gap is 2 grid units and nothing saturates); +0 elsewhere
    sl = rig.slots.cpu().numpy().reshape(-1, SB(k))
    dense = _decode_topk_fp4(rig.slots.view(-1, SB(k)), k).cpu().numpy()
    x = np.zeros(dense.size, dtype=F)
    for i, o in enumerate(np.cumsum([0] + [-(-n // N) * N for n in NUMELS[:-1]])):
        d = theta[i] - inner[i]
        x[o:o + d.size] = d + resid[i] if ef else d
    for c, xc in enumerate(x.reshape(-1, N).astype(np.float64)):
        idx = np.sort(np.argsort(-np.abs(xc), kind="stable")[:k])
        assert ((sl[c, 16:].view(np.uint16) & 4095) == idx).all(), c
        bound = np.ldexp(1.0, np.repeat(sl[c, :8].astype(int), 32)[:k] - 127)
        assert (np.abs(dense[c, idx].astype(np.float64) - xc[idx]) <= bound).all(), c
        assert np.count_nonzero(np.delete(dense[c].view(np.uint32), idx)) == 0, c
    rig.tree.close()


_MID = np.array([6, .25, .75, 1.25, 1.75, 2.5, 3.5, 5]) / 8  # a 6 in every group: scale 2^-3
FP4_EDGE = {  # name -> (rng, k) -> one chunk
    # a group's entries span 2^7: the small ones are sent as code 0 and stay whole in the residual
    "span": lambda r, k: _put(r.choice(N, k, replace=False), np.tile([1.0, -2.0 ** -7], k // 2)),
    "midpoints": lambda r, k: _put(np.sort(r.choice(N, k, replace=False)),  # ties to the even code
                                   np.tile(_MID, k // 8) * r.choice([-1.0, 1.0], k)),
    # 20 non-zeros high up: entry group 0 is zeros only (E = 0), -0 among them
    "few": lambda r, k: _put(np.r_[5, r.choice(np.arange(2000, N), 20, replace=False)],
                             [-0.0] + [1.5] * 20),
    "denormals": EDGE["denormals"],
    "nan_inf": EDGE["nan_inf"],  # NaN at 77, -Inf at 3001: entry groups 0 and 1
}


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("name", list(FP4_EDGE))
def test_quantiser_edge_cases(name, misaligned):
    k, rng = 64, np.random.default_rng(5)
    rig = _Rig(k, misaligned, [N])
    theta, inner = [FP4_EDGE[name](rng, k).astype(F)], [np.zeros(N, dtype=F)]  # x - (+0) = x
    resid = [np.zeros(N, dtype=F)]
    with np.errstate(all="ignore"):
        want_s, want_r = _expect(theta, inner, resid, k)
    ent, sc = want_s[16:].view(np.uint16), want_s[:8].tolist()
    if name == "span":
        assert (ent >> 12 == 0).sum() == k // 2 and np.count_nonzero(want_r[0]) == k // 2
    if name == "midpoints":  # 6, then the seven midpoints: 0.25 -> 0, 0.75 -> 1 -> 2, ..., 5 -> 4 -> 6
        assert ((ent >> 12) & 7).tolist() == [7, 0, 2, 2, 4, 4, 6, 6] * (k // 8)
    assert name != "few" or (sc == [0, 125] + [0] * 6 and theta[0].view(np.uint32)[5] == 1 << 31)
    assert name != "nan_inf" or sc == [255, 255] + [0] * 6
    res = rig.encode(theta, inner, resid, "whole")
    _same(rig.slots, want_s, name)
    rig.check(res, want_r, (name, "residual"))
    rig.encode(theta, inner, None, "whole")  # no residual add: -0 reaches the selection as it is
    _same(rig.slots, _expect(theta, inner, None, k)[0], (name, "plain"))
    rig.tree.close()


@pytest.mark.parametrize("ef", [False, True])
@pytest.mark.parametrize("n,divisor", [(1, 1), (2, 2), (3, 3), (3, 1)])
def test_topk_fp4_reduce_matches_the_restatement(n, divisor, ef):
    k, m, rng = 64, 3, np.random.default_rng(10 * n + divisor)
    shared = rng.choice(N, 40, replace=False)  # overlapping and disjoint indices
    slots = []
    for r in range(n):
        for j in range(m):
            x = (_decades(rng, N) * F(1e-3)).astype(F)
            x[shared] = rng.standard_normal(40).astype(F)
            x[rng.choice(N, 30, replace=False)] = rng.standard_normal(30).astype(F)
            slots.append(tq.select(x, k, False)[0] if (r, j) != (0, 1) else np.zeros(SB(k), np.uint8))
    recv = np.concatenate(slots)
    res0 = _decades(rng, m * N) if ef else None
    want, want_r = tq.reduce_slots(recv, n, m, divisor, k, res0)
    d_recv = torch.from_numpy(recv).to(DEV)
    out = d_recv if n == 1 else torch.full((m * SB(k),), 0xEE, dtype=torch.uint8, device=DEV)
    res = torch.from_numpy(res0).to(DEV) if ef else None
    K.topk_fp4_reduce(d_recv, n, m, divisor, res, k, out)
    _same(out, want, (n, divisor, ef))
    assert not ef or tq.same_bits(res.cpu().numpy(), want_r)


@pytest.mark.parametrize("write_inner", [True, False])
@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("rule", ["sgd0", "nesterov", "adamw"])
def test_unpack_topk_fp4_equals_decode_then_unpack(rule, misaligned, write_inner):
    k, rng = 64, np.random.default_rng(23)
    rigs = [_Rig(k, misaligned), _Rig(k, misaligned)]  # the fused pass; decode + the fp32 pass
    slots, _ = _expect([_decades(rng, n) for n in NUMELS], [np.zeros(n, dtype=F) for n in NUMELS],
                       None, k)
    dense = _decode_topk_fp4(torch.from_numpy(slots).to(DEV).view(-1, SB(k)), k).cpu().numpy()
    assert tq.same_bits(dense, np.stack([tq.decode(s, k) for s in slots.reshape(-1, SB(k))]))
    wire, c = [], 0
    for n in NUMELS:
        nch = -(-n // N)
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
            (K.unpack_adamw_topk_fp4(rig.tree, ALL, src, k, th, m1, m2, ADAM, slot) if fused else
             K.unpack_adamw(rig.tree, ALL, src, 1, th, m1, m2, ADAM, slot))
        else:
            (K.unpack_sgd_topk_fp4(rig.tree, ALL, src, k, th, m1, *hp, slot) if fused else
             K.unpack_sgd(rig.tree, ALL, src, 1, th, m1, *hp, slot))
        torch.cuda.synchronize()
        outs.append([a.cpu().numpy() for a in (th, m1, m2, *rig.inner)])
    for a, b in zip(*outs):  # padding sentinels included: whole arenas, byte for byte
        assert a.tobytes() == b.tobytes()
    assert (outs[0][0].view(np.uint32)[rigs[0].pad] == base.SENTINEL).all()
    for rig in rigs:
        rig.tree.close()


def _worker(rank, world, port, rule):
    # test_topk_gpu's worker builds wire="topk", topk=64 with error feedback and checks θ, inner,
    # .grad and both residuals against tk.TopkExchange: here with the 4-bit values asked for
    # through the environment and this codec's exchange as its reference
    os.environ["DILOCO_OUTER_TOPK_VALUES"] = "fp4"
    base.tk = tq
    base._worker(rank, world, port, rule)


@pytest.mark.parametrize("rule", ["sgd", "adamw"])
def test_dropin_topk_fp4_wire_two_peers_on_gpu(rule):
    """Two gloo processes on the one GPU, placement="device", wire="topk", topk=64,
    topk_values="fp4", three outer steps, asserted inside each rank."""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mp.spawn(_worker, args=(2, port, rule), nprocs=2, join=True)
