"""The fused AdamW outer step after the int8 exchange, without a GPU.

gloo CPU ranks on the checker backend (tests/q8_adamw_oracle_kernels.py), spawned like
tests/test_shard_adamw_cpu.py's: the reference's four calls (src/train.py:263-269) with
DILOCO_OUTER_ADAMW=fused and wire="int8" on the micro tree in three or more buckets, both
placements, at 2 and 3 peers, against tests/adamw_restatement.py's AdamWState stepped on the
oracle's restatement of the int8 exchange (oracle.q8_average: dl_q8_reduce sums in rank order,
so it is exact at every n) -- θ, the inner params, .grad, exp_avg, exp_avg_sq and the step
counts bit for bit and equal on every rank. Fused mode must take dl_unpack_adamw_q8 (one per
bucket, no dl_unpack_adamw); eager mode (DILOCO_OUTER_FUSED=0: decode, then dl_unpack_adamw)
is the second witness of the same bytes."""
import os
import socket
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import PKG, REPO
from diloco_amd import _lib

HYPER = dict(lr=0.01, betas=(0.9, 0.95), weight_decay=0.1)
STEPS = 3
KEYS = ("theta", "inner", "grad", "exp_avg", "exp_avg_sq")


class _Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _host(ts):
    return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in ts])


def _worker(rank, world, port, placement, fused, amsgrad, out):
    for p in (PKG, REPO, os.path.join(REPO, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    torch.set_num_threads(1)
    import expect

    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      DILOCO_OUTER_BUCKET_ELEMS=str(expect.MICRO_Q8_CAP),
                      DILOCO_OUTER_ADAMW="fused", DILOCO_OUTER_FUSED="1" if fused else "0")
    for v in ("DILOCO_OUTER_EXCHANGE", "DILOCO_DP_EXCHANGE", "DILOCO_OUTER_WIRE"):
        os.environ.pop(v, None)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank,
                            world_size=world)
    from adamw_restatement import AdamWState
    from diloco_amd import kernels, synth
    from diloco_amd.comm import TrainingComm
    from diloco_amd.optim import OuterAdamW
    from diloco_amd.trees import get_tree
    from diloco_amd.utils import (compute_pseudo_gradient, get_optimizer, get_outer_model,
                                  outer_mirror, sync_inner_model)
    from diloco_amd.world import World
    from oracle import oracle
    from q8_adamw_oracle_kernels import Q8AdamWOracleKernels

    k = Q8AdamWOracleKernels()
    kernels.set_default_kernels(k)
    world_ = World.from_default_group(1)
    spec = get_tree("micro")
    numels = spec.numels()
    shapes = [s for _, s in spec.params()]
    theta0 = synth.outer_tree(numels, spec.init_spec())
    inner = torch.nn.Module()
    inner.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(v.copy()).view(s))
                                       for v, s in zip(theta0, shapes)])
    outer = get_outer_model(inner, placement=placement, wire="int8")
    opt = get_optimizer(outer, _Cfg(type="AdamW", **HYPER))
    assert type(opt) is OuterAdamW
    if amsgrad:
        opt.param_groups[0]["amsgrad"] = True
    comm = TrainingComm(world_, (1, 1, 32), None)
    ref = AdamWState(theta0, **HYPER)
    m = outer_mirror(outer)
    dev = getattr(m, "dev", m)
    counts = [c1 - c0 for c0, c1 in dev.tree.bucket_chunks]
    rec = {"n_buckets": np.array(dev.tree.n_buckets), "mirror": np.array(type(m).__name__)}

    def four_calls(s, theta_ref):
        vals = [synth.inner_tree(theta_ref, s, r) for r in range(world)]
        with torch.no_grad():
            for p, v in zip(inner.parameters(), vals[rank]):
                p.copy_(torch.from_numpy(v).view(p.shape))
        n0 = len(k.calls)
        compute_pseudo_gradient(inner, outer)
        comm.sync_gradients(outer)
        opt.step()
        sync_inner_model(outer, inner)
        rec[f"calls_s{s}"] = np.array([c[0] for c in k.calls[n0:]])
        rec[f"buckets_s{s}"] = np.array([c[1] for c in k.calls[n0:]
                                         if c[0] == "unpack_adamw_q8"], dtype=np.int64)
        deltas = [[oracle.delta(t, i) for t, i in zip(theta_ref, v)] for v in vals]
        return oracle.q8_average(deltas, numels, counts)

    if amsgrad:  # a fallback still falls back: torch's own step body on the decoded .grad
        avg = four_calls(1, ref.theta)
        stock_p = [torch.nn.Parameter(torch.from_numpy(t.copy())) for t in theta0]
        stock = torch.optim.AdamW(stock_p, amsgrad=True, **HYPER)
        for p, g in zip(stock_p, avg):
            p.grad = torch.from_numpy(g.copy())
        stock.step()
        ps = list(outer.parameters())
        rec["theta"] = _host(ps)
        rec["inner"] = _host(inner.parameters())
        rec["ref_theta"] = _host(stock_p)
        rec["state_keys"] = np.array(sorted(opt.state[ps[0]]))
        np.savez(os.path.join(out, f"r{rank}.npz"), **rec)
        dist.barrier()
        dist.destroy_process_group()
        return

    def outer_step(s):
        avg = four_calls(s, ref.theta)
        ref.step_grads(avg)
        ps = list(outer.parameters())
        st = [opt.state[p] for p in ps]
        rec[f"theta_s{s}"] = _host(ps)
        rec[f"inner_s{s}"] = _host(inner.parameters())
        rec[f"grad_s{s}"] = _host(p.grad for p in ps)  # decoded from the slots after the step
        rec[f"exp_avg_s{s}"] = _host(x["exp_avg"] for x in st)
        rec[f"exp_avg_sq_s{s}"] = _host(x["exp_avg_sq"] for x in st)
        rec[f"step_s{s}"] = np.array([float(x["step"]) for x in st])
        rec[f"ref_theta_s{s}"] = rec[f"ref_inner_s{s}"] = np.concatenate(ref.theta)
        rec[f"ref_grad_s{s}"] = np.concatenate(avg)
        rec[f"ref_exp_avg_s{s}"] = np.concatenate(ref.m)
        rec[f"ref_exp_avg_sq_s{s}"] = np.concatenate(ref.v)

    outer_step(1)
    ps = list(outer.parameters())
    arena = m._adam_views if hasattr(m, "_adam_views") else (dev._views["exp_avg"],
                                                             dev._views["exp_avg_sq"])
    rec["state_is_arena_views"] = np.array(
        arena is not None
        and all(opt.state[p]["exp_avg"] is a for p, a in zip(ps, arena[0]))
        and all(opt.state[p]["exp_avg_sq"] is a for p, a in zip(ps, arena[1])))
    for s in range(2, STEPS + 1):
        outer_step(s)
    # state_dict() loads into a stock AdamW and back; the step after still matches
    sd = opt.state_dict()
    stock = torch.optim.AdamW([torch.nn.Parameter(p.detach().cpu().clone())
                               for p in outer.parameters()], **HYPER)
    stock.load_state_dict(sd)
    sp = stock.param_groups[0]["params"]
    rec["stock_exp_avg"] = _host(stock.state[p]["exp_avg"] for p in sp)
    rec["stock_exp_avg_sq"] = _host(stock.state[p]["exp_avg_sq"] for p in sp)
    rec["stock_step"] = np.array([float(stock.state[p]["step"]) for p in sp])
    opt.load_state_dict(stock.state_dict())
    outer_step(STEPS + 1)
    np.savez(os.path.join(out, f"r{rank}.npz"), **rec)
    dist.barrier()
    dist.destroy_process_group()


def _run(world, placement, fused=True, amsgrad=False):
    out = tempfile.mkdtemp(prefix="dl_q8_adamw_")
    # forked workers, as tests/test_dist_gloo.py: CPU only, no HIP state to inherit
    mp.start_processes(_worker, args=(world, _free_port(), placement, fused, amsgrad, out),
                       nprocs=world, join=True, start_method="fork")
    return [dict(np.load(os.path.join(out, f"r{r}.npz"))) for r in range(world)]


@pytest.mark.parametrize("placement", [None, "device"])
@pytest.mark.parametrize("world", [2, 3])
def test_four_calls_on_the_int8_wire_match_the_restatement(world, placement):
    recs = _run(world, placement)
    eager = _run(world, placement, fused=False)
    for rec, erec in zip(recs, eager):
        nb = int(rec["n_buckets"])
        assert nb >= 3
        assert str(rec["mirror"]) == ("DeviceOuterMirror" if placement else "LazyHostOuterMirror")
        assert bool(rec["state_is_arena_views"])
        for s in range(1, STEPS + 2):
            # the fused plan: one dl_unpack_adamw_q8 per bucket, no other AdamW pass
            calls = [str(c) for c in rec[f"calls_s{s}"]]
            assert calls.count("unpack_adamw_q8") == nb, (s, calls)
            assert sorted(rec[f"buckets_s{s}"].tolist()) == list(range(nb)), s
            assert not [c for c in calls if "adamw" in c and c != "unpack_adamw_q8"], (s, calls)
            ecalls = [str(c) for c in erec[f"calls_s{s}"]]
            assert "unpack_adamw_q8" not in ecalls and "unpack_adamw" in ecalls, (s, ecalls)
            for key in KEYS:
                want = rec[f"ref_{key}_s{s}"].tobytes()
                assert rec[f"{key}_s{s}"].tobytes() == want, (key, s)
                assert recs[0][f"{key}_s{s}"].tobytes() == want, (key, s)
                assert erec[f"{key}_s{s}"].tobytes() == want, ("eager", key, s)
            assert (rec[f"step_s{s}"] == float(s)).all()
            assert (erec[f"step_s{s}"] == float(s)).all()
        for key in ("exp_avg", "exp_avg_sq"):
            assert rec[f"stock_{key}"].tobytes() == rec[f"ref_{key}_s{STEPS}"].tobytes(), key
        assert (rec["stock_step"] == float(STEPS)).all()


@pytest.mark.parametrize("placement", [None, "device"])
def test_a_fallback_still_falls_back_on_the_int8_wire(placement):
    """amsgrad is outside the fused contract: torch's own step body runs on the decoded .grad."""
    recs = _run(2, placement, amsgrad=True)
    for rec in recs:
        calls = [str(c) for c in rec["calls_s1"]]
        assert not [c for c in calls if "adamw" in c], calls
        assert "max_exp_avg_sq" in [str(x) for x in rec["state_keys"]]
        assert rec["theta"].tobytes() == rec["ref_theta"].tobytes()
        assert rec["inner"].tobytes() == rec["ref_theta"].tobytes()
        assert rec["theta"].tobytes() == recs[0]["theta"].tobytes()


def test_unpack_adamw_q8_argument_checks():
    """dl_unpack_adamw_q8 rejects bad arguments before touching a device."""
    sc = (0.999, 0.1, 0.95, 0.05, -0.1, 0.2236, 1e-8)
    with pytest.raises(_lib.DilocoHipError, match="null tree"):
        _lib.call("dl_unpack_adamw_q8", None, 0, 64, 128, 192, 256, *sc, -1, None)
