"""The outer step on the gathered top-k slots on the GPU, bit for bit: the fused pass against
dl_unpack_avg_topk[_fp4]_ag into a packed fp32 wire followed by dl_unpack_sgd / dl_unpack_adamw,
and the drop-in calls at two peers against the restated exchange. Rig and inputs of
test_gradsync_topk_gpu.py and test_topk_ag_gpu.py; the rig's guarded tensors are the inner model."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import topk_ag_restatement as ag
import topk_restatement as tk
from conftest import PKG, REPO
from diloco_amd import _lib, synth
from diloco_amd.kernels import HipKernels, adamw_scalars
from diloco_amd.plan import SLOT_GRAD, SLOT_INNER
from diloco_amd.trees import get_tree
from gradsync_fp4_inputs import NUMELS
from oracle import oracle
from test_gradsync_topk_gpu import NAN_BITS, _Rig
from test_topk_ag_gpu import REFS, VALUES, peers  # noqa: F401  (peers: the module's fixture)

pytestmark = pytest.mark.gpu
DEV, F, ALL, K = "cuda:0", np.float32, _lib.ALL_BUCKETS, HipKernels()
ADAM = adamw_scalars(0.01, 0.9, 0.95, 0.1, 1e-8, 2)
RULES = {"sgd0": (0.7, 0.0, False, False), "nesterov": (0.7, 0.9, True, False), "adamw": None}


@pytest.fixture(scope="module")
def start():
    """θ, two state arenas (the second non-negative) and the inner model before the step; read only."""
    rng = np.random.default_rng(77)
    return [[f(rng.standard_normal(n)).astype(F) for n in NUMELS] for f in (np.copy, np.copy, np.abs, np.copy)]


@VALUES
@pytest.mark.parametrize("mode", ["whole", "buckets"])
@pytest.mark.parametrize("write_inner", [True, False], ids=["inner", "no_inner"])
@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("k", [8, 64, 256])
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("rule", list(RULES))
def test_fused_pass_equals_decode_then_step(peers, start, rule, n, k, misaligned, write_inner, mode, values):  # noqa: F811
    per, vals = peers[values, k]
    rig, fp4 = _Rig(k, values, misaligned, mode), values == "fp4"
    rig.tree.bind(SLOT_INNER, rig.grads, torch.cuda.current_stream().cuda_stream)
    slot = SLOT_INNER if write_inner else -1

    def packed(tensors):
        a = np.full(rig.tree.total, NAN_BITS, dtype=np.uint32).view(F)
        for o, t in zip(rig.offs, tensors):
            a[o:o + t.size] = t
        return torch.from_numpy(a).to(DEV)

    wire = packed([np.zeros(t, dtype=F) for t in NUMELS])
    rig.tree.bind(SLOT_GRAD, [wire[o:o + t] for o, t in zip(rig.offs, NUMELS)],
                  torch.cuda.current_stream().cuda_stream)
    outs = []
    for fused in (True, False):
        for d, i in zip(rig.grads, start[3]):
            d.copy_(torch.from_numpy(i))
        th, m1, m2 = packed(start[0]), packed(start[1]), packed(start[2])
        for b in ([ALL] if mode == "whole" else reversed(range(rig.tree.n_buckets))):
            c0, c1 = (0, rig.nch) if b == ALL else rig.tree.bucket_chunks[b]
            host = np.concatenate([p[c0 * rig.S:c1 * rig.S] for p in per[:n]])
            src = (torch.from_numpy(host).to(DEV), n, c1 - c0, k)
            if not fused:
                K.unpack_avg_topk_ag(rig.tree, b, *src, SLOT_GRAD, fp4=fp4)
            if rule == "adamw":
                (K.unpack_adamw_topk_ag(rig.tree, b, *src, th, m1, m2, ADAM, slot, fp4=fp4) if fused else
                 K.unpack_adamw(rig.tree, b, wire, 1, th, m1, m2, ADAM, slot))
            else:
                (K.unpack_sgd_topk_ag(rig.tree, b, *src, th, m1, *RULES[rule], slot, fp4=fp4) if fused else
                 K.unpack_sgd(rig.tree, b, wire, 1, th, m1, *RULES[rule], slot))
            torch.cuda.synchronize()
            assert src[0].cpu().numpy().tobytes() == host.tobytes()  # only read
        outs.append([a.cpu().numpy() for a in (th, m1, m2, *rig.grads)])
    for a, b in zip(*outs):  # whole arenas, padding sentinels included, byte for byte
        assert a.tobytes() == b.tobytes()
    theta = outs[0][0]
    assert (theta.view(np.uint32)[rig.pad] == NAN_BITS).all()
    g = wire.cpu().numpy()
    assert all(tk.same_bits(g[o:o + t], v) for o, t, v in zip(rig.offs, NUMELS, vals[n]))
    want_inner = [theta[o:o + t] for o, t in zip(rig.offs, NUMELS)] if write_inner else start[3]
    assert tk.same_bits(np.concatenate(outs[0][3:]), np.concatenate(want_inner))
    assert not tk.same_bits(theta[~rig.pad], np.concatenate(start[0]))
    rig.guards_hold()
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
                      DILOCO_OUTER_BUCKET_ELEMS=str(expect.MICRO_Q8_CAP), DILOCO_COLLECTIVE_READ_TIMEOUT="10")
    for v in [v for v in os.environ if v.startswith(("DILOCO_OUTER_TOPK", "DILOCO_OUTER_EXCHANGE", "DILOCO_OUTER_WIRE",
                                                     "DILOCO_OUTER_FUSED", "DILOCO_DP_EXCHANGE"))]:
        os.environ.pop(v)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    from adamw_restatement import AdamWState
    from diloco_amd.comm import TrainingComm
    from diloco_amd.utils import (compute_pseudo_gradient, get_optimizer, get_outer_model, outer_mirror,
                                  q8_error_feedback_state, sync_inner_model)
    from diloco_amd.world import World

    spec = get_tree("micro")
    numels, shapes = spec.numels(), [s for _, s in spec.params()]
    theta0 = synth.outer_tree(numels, spec.init_spec())
    comm = TrainingComm(World.from_default_group(1), (1, 1, 32), None)

    def flat(ts):
        return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in ts])
    for values, ref in REFS.items():
        inner = torch.nn.Module()
        inner.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(v.copy()).view(s))
                                           for v, s in zip(theta0, shapes)])
        outer = get_outer_model(inner, placement="device", wire="topk", topk=64, topk_values=values,
                                topk_exchange="gather")  # EF: on by default
        inner = inner.to(DEV)
        opt = get_optimizer(outer, SimpleNamespace(type="SGD" if rule == "sgd" else "AdamW",
                                                   **(SGD if rule == "sgd" else ADAMW)))
        adam = AdamWState(theta0, **ADAMW)
        theta, buf = [t.copy() for t in theta0], [np.empty_like(t) for t in theta0]
        res = [[np.zeros(n, dtype=F) for n in numels] for _ in range(world)]
        for s in (1, 2, 3):
            vals = [synth.inner_tree(theta, s, r) for r in range(world)]
            with torch.no_grad():
                for p, v in zip(inner.parameters(), vals[rank]):
                    p.copy_(torch.from_numpy(v).view(p.shape))
            compute_pseudo_gradient(inner, outer)
            comm.sync_gradients(outer)
            opt.step()
            sync_inner_model(outer, inner)
            enc = [[ref.encode_tensor(oracle.delta(t, i), 64, r) for t, i, r in zip(theta, v, rs)]
                   for v, rs in zip(vals, res)]
            avg = ag.average_tensors(ref, [np.concatenate([sl for sl, _ in e]) for e in enc], 64, numels)
            res = [[r for _, r in e] for e in enc]
            if rule == "sgd":
                for t in range(len(theta)):
                    oracle.sgd(theta[t], buf[t], avg[t], SGD["lr"], SGD["momentum"], True, s == 1)
            else:
                adam.step_grads(avg)
                theta = adam.theta
            torch.cuda.synchronize()
            assert flat(outer.parameters()).tobytes() == np.concatenate(theta).tobytes(), (values, s)
            assert flat(inner.parameters()).tobytes() == np.concatenate(theta).tobytes(), (values, s)
            assert tk.same_bits(flat([p.grad for p in outer.parameters()]), np.concatenate(avg)), (values, s)
        dev = getattr(outer_mirror(outer), "dev", outer_mirror(outer))
        assert dev.tree.n_buckets >= 3 and dev.topk_gather
        st = q8_error_feedback_state(outer)
        got = st["encode"].cpu().numpy()
        got = np.concatenate([got[o:o + n] for o, n in zip(dev.offs, numels)])
        assert tk.same_bits(got, np.concatenate(res[rank])) and got.any() and st["reduce"] == []
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("rule", ["sgd", "adamw"])
def test_dropin_topk_gather_two_peers_on_gpu(rule):
    """Two gloo processes on the one GPU, placement="device", wire="topk", topk_exchange="gather",
    both topk_values, three outer steps: θ, inner, .grad and the encoder's residual equal the
    restatement's on both ranks (asserted inside each rank; a failing rank fails the spawn)."""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mp.spawn(_worker, args=(2, port, rule), nprocs=2, join=True)
