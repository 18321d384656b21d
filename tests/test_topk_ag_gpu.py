"""The top-k wires' all-gather exchange on the GPU, bit for bit; rig of test_gradsync_topk_gpu.py."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import clip_restatement as cr
import topk_ag_restatement as ag
import topk_fp4_restatement as tq
import topk_restatement as tk
from conftest import PKG, REPO
from diloco_amd import _lib
from diloco_amd.gradsync import GradSync, slot_wire_bytes
from diloco_amd.kernels import HipKernels
from diloco_amd.plan import SLOT_GRAD
from gradsync_fp4_inputs import CAP, NUMELS, groupwise, special
from test_gradsync_topk_gpu import CASES, PART_SENTINEL, _Rig, _params, _set_grads, tied

pytestmark = pytest.mark.gpu
DEV, F, ALL, K = "cuda:0", np.float32, _lib.ALL_BUCKETS, HipKernels()
REFS = {"f32": tk, "fp4": tq}
VALUES = pytest.mark.parametrize("values", list(REFS))


@pytest.fixture(scope="module")
def peers():
    """(values, k) -> (three peers' slots, a NaN and an Inf among the entries (fp4 values: the Inf's
    group decodes to NaN), the restated average per peer count); read only."""
    out = {}
    for values, ref in REFS.items():
        for k, _mode, _make in CASES:
            S = slot_wire_bytes("topk", k, values)
            per = [np.concatenate([ref.encode_tensor(t, k)[0] for t in g])
                   for g in (special(21), tied(22), groupwise(23))]
            for p in per:
                p[3 * S:4 * S] = 0
            vals = {n: ag.average_tensors(ref, per[:n], k, NUMELS) for n in (1, 2, 3)}
            flat = np.concatenate(vals[2])
            assert np.isnan(flat).any() and (values == "fp4" or np.isinf(flat).any()) and not vals[3][3].any()
            out[values, k] = per, vals
    return out


@VALUES
@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("sumsq", [False, True], ids=["no_partials", "partials"])
@pytest.mark.parametrize("k,mode", [c[:2] for c in CASES], ids=[f"k{c[0]}-{c[1]}" for c in CASES])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_unpack_avg_topk_ag_matches_the_restatement(peers, k, mode, n, sumsq, misaligned, values):
    per, vals = peers[values, k]
    rig = _Rig(k, values, misaligned, mode)
    partials = torch.full((rig.nch,), PART_SENTINEL, dtype=torch.float64, device=DEV)
    for b in ([ALL] if mode != "buckets" else reversed(range(rig.tree.n_buckets))):
        c0, c1 = (0, rig.nch) if b == ALL else rig.tree.bucket_chunks[b]
        host = np.concatenate([p[c0 * rig.S:c1 * rig.S] for p in per[:n]])
        dev = torch.from_numpy(host).to(DEV)
        K.unpack_avg_topk_ag(rig.tree, b, dev, n, c1 - c0, k, SLOT_GRAD, partials if sumsq else None,
                             fp4=values == "fp4")
        torch.cuda.synchronize()
        assert dev.cpu().numpy().tobytes() == host.tobytes()  # only read
        if b != ALL:  # a bucket launch writes exactly its chunk range of the partial sums
            p = partials.cpu().numpy()
            assert (p[:c0] == PART_SENTINEL).all() and (p[c0:c1] != PART_SENTINEL).all() == sumsq
    assert all(tk.same_bits(d.cpu().numpy(), v) for d, v in zip(rig.grads, vals[n]))
    rig.guards_hold()
    again = torch.full_like(partials, PART_SENTINEL)
    if sumsq:  # the restatement's, and dl_grad_sumsq's on the destination afterwards
        K.grad_sumsq(rig.tree, ALL, SLOT_GRAD, again)
        assert tk.same_bits(partials.cpu().numpy(), cr.tree_partials(vals[n]))
    assert tk.same_bits(partials.cpu().numpy(), again.cpu().numpy())
    rig.tree.close()


def _restated(ref, by_rank, res, k):  # one sync: (the averaged tensors, the ranks' new residuals)
    enc = [[ref.encode_tensor(x, k, r) for x, r in zip(g, rs)] for g, rs in zip(by_rank, res)]
    want = ag.average_tensors(ref, [np.concatenate([s for s, _ in e]) for e in enc], k, NUMELS)
    return want, [[r for _, r in e] for e in enc]


@VALUES
def test_gradsync_gather_one_replica_matches_the_restatement(values):
    ps = _params(groupwise(40))
    gs = GradSync(ps, None, 1, wire_dtype="topk", topk=64, topk_values=values, bucket_cap_elems=CAP,
                  topk_exchange="gather")
    res = [[np.zeros(n, dtype=F) for n in NUMELS]]
    for s in (1, 2):  # the second sync carries a residual, and clips with the free norm
        _set_grads(ps, tied(40 + s))
        want, res = _restated(REFS[values], [tied(40 + s)], res, 64)
        if s == 1:
            assert gs.sync() is None
        else:
            max_norm = 0.5 * float(cr.norm_and_coef(want, 1.0)[0])
            norm, coef, want = cr.clip(want, max_norm)
            assert coef != 1 and np.float32(gs.sync(max_norm).item()).tobytes() == norm.tobytes()
        torch.cuda.synchronize()
        assert all(p.grad.cpu().numpy().tobytes() == w.tobytes() for p, w in zip(ps, want)), s
    assert gs.topk_gather and gs.error_feedback and gs.q_residual_red is None
    assert gs.q8_ef_state()["reduce"] == [] and gs.q8_ef_state()["encode"].any()
    gs.close()


def _worker(rank, world, port):
    for p in (PKG, REPO, os.path.join(REPO, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(DILOCO_DP_BACKEND="gloo", DILOCO_COLLECTIVE_READ_TIMEOUT="10")
    for v in [v for v in os.environ if v.startswith("DILOCO_DP_") and v != "DILOCO_DP_BACKEND"]:
        os.environ.pop(v)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    from diloco_amd import comm
    from diloco_amd.world import World

    tc = comm.TrainingComm(World.from_default_group(1), (1, 1, 32), None)
    for values, ref in REFS.items():  # the knobs, patched
        comm.DP_WIRE, comm.DP_TOPK, comm.DP_TOPK_VALUES, comm.DP_TOPK_EXCHANGE = "topk", 32, values, "gather"
        model = torch.nn.Module()
        model.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(n, device=DEV)) for n in NUMELS])
        res = [[np.zeros(n, dtype=F) for n in NUMELS] for _ in range(world)]
        for s in (1, 2):
            by_rank = [groupwise(100 * s + r) for r in range(world)]
            _set_grads(list(model.parameters()), by_rank[rank])
            assert tc.sync_gradients(model) is None
            torch.cuda.synchronize()
            want, res = _restated(ref, by_rank, res, 32)
            got = np.concatenate([p.grad.cpu().numpy() for p in model.parameters()])
            assert got.tobytes() == np.concatenate(want).tobytes(), (values, s)
        gs = tc.dp._grad_syncs[id(model)]
        st, enc = gs.q8_ef_state(), gs.q8_ef_state()["encode"].cpu().numpy()
        enc = np.concatenate([enc[int(o):int(o) + n] for o, n in zip(gs.tree.seg_off, NUMELS)])
        assert tk.same_bits(enc, np.concatenate(res[rank])) and enc.any() and st["reduce"] == []
        assert gs.topk_gather and not gs.local and gs.q_residual_red is None
    dist.barrier()
    dist.destroy_process_group()


def test_training_comm_topk_gather_two_peers_on_gpu():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mp.spawn(_worker, args=(2, port), nprocs=2, join=True)
