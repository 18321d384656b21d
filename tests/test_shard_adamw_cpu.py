"""The fused AdamW outer step on the sharded and rank-order exchanges, without a GPU.

gloo CPU ranks on the checker backend (tests/shard_adamw_oracle_kernels.py), spawned like
tests/test_dist_gloo.py's: the reference's four calls (src/train.py:263-269) with
DILOCO_OUTER_ADAMW=fused on the micro tree in several buckets, both placements, against
tests/adamw_restatement.py's AdamWState over the rank-order fp32 average -- θ, the inner
params, .grad, exp_avg and exp_avg_sq bit for bit and equal on every rank. At two peers a + b
has one order, so the sharded exchange (a SUM reduce_scatter) is exact too; at three only the
rank-order exchange is compared."""
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


class _Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _host(ts):
    return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in ts])


def _worker(rank, world, port, exchange, placement, out):
    for p in (PKG, REPO, os.path.join(REPO, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    torch.set_num_threads(1)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      DILOCO_OUTER_BUCKET_ELEMS="4096", DILOCO_OUTER_ADAMW="fused")
    os.environ.pop("DILOCO_OUTER_EXCHANGE", None)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank,
                            world_size=world)
    import diloco_amd.comm as comm_mod
    from adamw_restatement import AdamWState
    from diloco_amd import kernels, synth
    from diloco_amd.comm import TrainingComm
    from diloco_amd.optim import OuterAdamW
    from diloco_amd.trees import get_tree
    from diloco_amd.utils import (compute_pseudo_gradient, get_optimizer, get_outer_model,
                                  outer_mirror, sync_inner_model)
    from diloco_amd.world import World
    from shard_adamw_oracle_kernels import ShardAdamWOracleKernels

    k = ShardAdamWOracleKernels()
    kernels.set_default_kernels(k)
    comm_mod.DP_EXCHANGE = "a2a" if exchange == "a2a" else "rccl"
    world_ = World.from_default_group(1)
    spec = get_tree("micro")
    shapes = [s for _, s in spec.params()]
    theta0 = synth.outer_tree(spec.numels(), spec.init_spec())
    inner = torch.nn.Module()
    inner.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(v.copy()).view(s))
                                       for v, s in zip(theta0, shapes)])
    outer = get_outer_model(inner, placement=placement,
                            exchange="sharded" if exchange == "sharded" else None)
    cfg = _Cfg(type="AdamW", **HYPER)
    opt = get_optimizer(outer, cfg)
    assert type(opt) is OuterAdamW
    comm = TrainingComm(world_, (1, 1, 32), None)
    ref = AdamWState(theta0, **HYPER)
    rec = {}

    def outer_step(s, read_state):
        vals = [synth.inner_tree(ref.theta, s, r) for r in range(world)]
        with torch.no_grad():
            for p, v in zip(inner.parameters(), vals[rank]):
                p.copy_(torch.from_numpy(v).view(p.shape))
        n0 = len(k.calls)
        compute_pseudo_gradient(inner, outer)
        comm.sync_gradients(outer)
        opt.step()
        sync_inner_model(outer, inner)
        rec[f"calls_s{s}"] = np.array([c[0] for c in k.calls[n0:]])
        _, avg = ref.step(vals)
        rec[f"theta_s{s}"] = _host(outer.parameters())
        rec[f"inner_s{s}"] = _host(inner.parameters())
        rec[f"grad_s{s}"] = _host(p.grad for p in outer.parameters())  # a collective read
        rec[f"ref_theta_s{s}"] = np.concatenate(ref.theta)
        rec[f"ref_grad_s{s}"] = np.concatenate(avg)
        if read_state:  # a collective read too: after it the state arenas are whole again
            st = [opt.state[p] for p in outer.parameters()]
            rec[f"exp_avg_s{s}"] = _host(x["exp_avg"] for x in st)
            rec[f"exp_avg_sq_s{s}"] = _host(x["exp_avg_sq"] for x in st)
            rec[f"ref_exp_avg_s{s}"] = np.concatenate(ref.m)
            rec[f"ref_exp_avg_sq_s{s}"] = np.concatenate(ref.v)
            rec[f"step_s{s}"] = np.array([float(x["step"]) for x in st])

    # step 2 runs on the state step 1 left sharded (nothing read it in between)
    for s in range(1, STEPS + 1):
        outer_step(s, read_state=s >= 2)
    m = outer_mirror(outer)
    dev = getattr(m, "dev", m)
    rec["n_buckets"] = np.array(dev.tree.n_buckets)
    rec["mirror"] = np.array(type(m).__name__)
    # a step whose state nobody reads; then, on every rank, state_dict() gathers it, and it
    # loads into a stock AdamW
    outer_step(STEPS + 1, read_state=False)
    rec["stale_after_step"] = np.array(dev._adam_stale)
    sd = opt.state_dict()
    rec["stale_after_state_dict"] = np.array(dev._adam_stale)
    stock = torch.optim.AdamW([torch.nn.Parameter(p.detach().cpu().clone())
                               for p in outer.parameters()], **HYPER)
    stock.load_state_dict(sd)
    ps = stock.param_groups[0]["params"]
    rec["stock_exp_avg"] = _host(stock.state[p]["exp_avg"] for p in ps)
    rec["stock_exp_avg_sq"] = _host(stock.state[p]["exp_avg_sq"] for p in ps)
    rec["stock_step"] = np.array([float(stock.state[p]["step"]) for p in ps])
    rec["ref_stock_exp_avg"] = np.concatenate(ref.m)
    rec["ref_stock_exp_avg_sq"] = np.concatenate(ref.v)
    # ... and back: the step after still matches
    opt.load_state_dict(stock.state_dict())
    outer_step(STEPS + 2, read_state=True)
    np.savez(os.path.join(out, f"r{rank}.npz"), **rec)
    dist.barrier()
    dist.destroy_process_group()


def _run(world, exchange, placement):
    out = tempfile.mkdtemp(prefix="dl_shard_adamw_")
    # forked workers, as tests/test_dist_gloo.py: CPU only, no HIP state to inherit
    mp.start_processes(_worker, args=(world, _free_port(), exchange, placement, out),
                       nprocs=world, join=True, start_method="fork")
    return [dict(np.load(os.path.join(out, f"r{r}.npz"))) for r in range(world)]


@pytest.mark.parametrize("placement", [None, "device"])
@pytest.mark.parametrize("exchange,world", [("sharded", 2), ("a2a", 2), ("a2a", 3)])
def test_four_calls_on_the_sharded_exchanges_match_the_restatement(exchange, world, placement):
    recs = _run(world, exchange, placement)
    kernel = "shard_adamw" if exchange == "sharded" else "shard_reduce_adamw"
    for rec in recs:
        nb = int(rec["n_buckets"])
        assert nb > 2
        assert str(rec["mirror"]) == ("DeviceOuterMirror" if placement else "LazyHostOuterMirror")
        for s in range(1, STEPS + 3):
            for key in ("theta", "grad"):
                assert rec[f"{key}_s{s}"].tobytes() == rec[f"ref_{key}_s{s}"].tobytes(), (key, s)
            assert rec[f"inner_s{s}"].tobytes() == rec[f"ref_theta_s{s}"].tobytes(), s
            for key in ("theta", "inner", "grad"):
                assert rec[f"{key}_s{s}"].tobytes() == recs[0][f"{key}_s{s}"].tobytes(), (key, s)
            # n_buckets shard-AdamW calls per step, no whole-tree AdamW pass
            calls = [str(c) for c in rec[f"calls_s{s}"]]
            assert calls.count(kernel) == nb, (s, calls)
            assert not [c for c in calls if "adamw" in c and c != kernel], (s, calls)
        for s in (2, 3, STEPS + 2):
            for key in ("exp_avg", "exp_avg_sq"):
                assert rec[f"{key}_s{s}"].tobytes() == rec[f"ref_{key}_s{s}"].tobytes(), (key, s)
                assert rec[f"{key}_s{s}"].tobytes() == recs[0][f"{key}_s{s}"].tobytes(), (key, s)
            assert (rec[f"step_s{s}"] == float(s)).all()
        # a sharded step leaves the state sharded; state_dict() gathers it
        assert bool(rec["stale_after_step"]) and not bool(rec["stale_after_state_dict"])
        for key in ("exp_avg", "exp_avg_sq"):
            assert rec[f"stock_{key}"].tobytes() == rec[f"ref_stock_{key}"].tobytes(), key
        assert (rec["stock_step"] == float(STEPS + 1)).all()


def test_shard_adamw_argument_checks():
    """dl_shard_adamw / dl_shard_reduce_adamw reject bad arguments before touching a device."""
    sc = (0.999, 0.1, 0.95, 0.05, -0.1, 0.2236, 1e-8)
    F32 = _lib.DL_F32
    for args, msg in [((16, F32, 2, 6, 32, 48, 64, None) + sc, "multiple of 4"),
                      ((16, F32, 0, 8, 32, 48, 64, None) + sc, "n_slices"),
                      ((16, 7, 2, 8, 32, 48, 64, None) + sc, "wire dtype"),
                      ((20, F32, 2, 8, 32, 48, 64, None) + sc, "aligned"),
                      ((16, F32, 2, 8, 36, 48, 64, None) + sc, "aligned"),
                      ((16, F32, 2, 8, 32, 52, 64, None) + sc, "aligned"),
                      ((16, F32, 2, 8, 32, 48, 64, 84) + sc, "aligned"),
                      ((16, F32, 2, 8, 32, None, 64, None) + sc, "exp_avg is null"),
                      ((16, F32, 2, 8, 32, 48, None, None) + sc, "exp_avg_sq is null")]:
        with pytest.raises(_lib.DilocoHipError, match=msg):
            _lib.call("dl_shard_reduce_adamw", *args, None)
    _lib.call("dl_shard_reduce_adamw", 16, F32, 2, 0, 32, 48, 64, None, *sc, None)  # empty
    for args, msg in [((16, F32, 0, 32, 48, 64, 8) + sc, "divisor"),
                      ((16, F32, 1, 32, 48, 64, -1) + sc, "n -1"),
                      ((16, 5, 1, 32, 48, 64, 8) + sc, "wire dtype"),
                      ((24, F32, 1, 32, 48, 64, 8) + sc, "aligned"),
                      ((16, F32, 1, 32, 44, 64, 8) + sc, "aligned"),
                      ((16, F32, 1, 32, None, 64, 8) + sc, "exp_avg is null"),
                      ((16, F32, 1, 32, 48, None, 8) + sc, "exp_avg_sq is null")]:
        with pytest.raises(_lib.DilocoHipError, match=msg):
            _lib.call("dl_shard_adamw", *args, None)
    _lib.call("dl_shard_adamw", 16, F32, 1, 32, 48, 64, 0, *sc, None)  # empty
