#!/usr/bin/env python3
"""The AdamW outer step on T125, one GPU, one peer: stock torch.optim.AdamW (DILOCO_OUTER_ADAMW
unset: dl_delta_pack on the first .grad read, then torch's single-tensor AdamW, on the host
twin for the default placement) against optim.OuterAdamW (DILOCO_OUTER_ADAMW=fused: one
dl_delta_pack_adamw pass), both placements, in one process and in interleaved order.

Each timed step is the reference's four calls (compute_pseudo_gradient, sync_gradients,
optimizer.step, sync_inner_model). The inner values are refilled before every step, outside the
timed window, so the deltas are never zero. Two clocks per step: the host clock around the four
calls ending in a device synchronise (the step's cost to the training loop; the stock host
placement computes on the CPU, which device events do not see) and device events on the
step's stream. Medians and means over the timed steps of every round.

In the same run: dl_delta_pack_adamw (36 B/param) and dl_delta_pack_sgd (28 B/param) launched
directly over the whole tree, interleaved, device events per launch; GB/s over the bytes the
algorithm needs and the fraction of the 8 TB/s HBM peak (bandwidth-bound: MI355X_MICROARCH).

    python tools/adamw_outer_bench.py [--rounds 3] [--steps 10] [--torch-host-steps 2]
                                      [--kernel-launches 30] [--tree t125] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from types import SimpleNamespace

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "diloco-swarm_amd"))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from diloco_amd import _lib, synth  # noqa: E402
from diloco_amd.comm import TrainingComm  # noqa: E402
from diloco_amd.kernels import HipKernels, adamw_scalars  # noqa: E402
from diloco_amd.plan import SLOT_INNER, PackedTree  # noqa: E402
from diloco_amd.trees import get_tree  # noqa: E402
from diloco_amd.utils import (compute_pseudo_gradient, get_optimizer, get_outer_model,  # noqa: E402
                              sync_inner_model)
from diloco_amd.world import World  # noqa: E402

HBM_PEAK = 8e12  # B/s
CFG = SimpleNamespace(type="AdamW", lr=0.01, weight_decay=0.1, betas=(0.9, 0.95))


def _stats(xs):
    return {"median": round(statistics.median(xs), 5), "mean": round(statistics.fmean(xs), 5),
            "min": round(min(xs), 5), "max": round(max(xs), 5), "n": len(xs)}


def _refill(inner, step):
    flat = [p.data.view(-1) for p in inner.parameters()]
    synth.inner_tree_device(flat, step, 0, out=flat)  # inner = θ + noise(step): nonzero deltas


def _four_calls(inner, outer, opt, comm):
    compute_pseudo_gradient(inner, outer)
    comm.sync_gradients(outer)
    opt.step()
    sync_inner_model(outer, inner)


def outer_steps(spec, dev, args):
    shapes = [s for _, s in spec.params()]
    comm = TrainingComm(World.from_default_group(1), (1, 1, spec.n_embd), None)
    setups = {}
    for placement in ("host", "device"):
        for knob in ("torch", "fused"):
            inner = torch.nn.Module()
            inner.ps = torch.nn.ParameterList([torch.nn.Parameter(t.view(s)) for t, s in zip(
                synth.outer_tree_device(spec, dev), shapes)])
            outer = get_outer_model(inner, "device" if placement == "device" else None)
            if knob == "fused":
                os.environ["DILOCO_OUTER_ADAMW"] = "fused"
            else:
                os.environ.pop("DILOCO_OUTER_ADAMW", None)  # the baseline: the knob unset
            opt = get_optimizer(outer, CFG)
            setups[placement, knob] = (inner, outer, opt, [0])
    res = {f"{p}_{k}": {"optimizer": type(v[2]).__name__, "wall_ms": [], "gpu_ms": []}
           for (p, k), v in setups.items()}

    def run(key, timed):
        inner, outer, opt, count = setups[key]
        count[0] += 1
        _refill(inner, count[0])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        _four_calls(inner, outer, opt, comm)
        e1.record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        if timed:
            r = res["_".join(key)]
            r["wall_ms"].append(round(wall, 5))
            r["gpu_ms"].append(round(e0.elapsed_time(e1), 5))

    for key in setups:  # warm up every shape the timed window uses
        for _ in range(2):
            run(key, False)
    for r in range(args.rounds):
        keys = list(setups)
        if r % 2:
            keys.reverse()
        for key in keys:
            n = args.torch_host_steps if key == ("host", "torch") else args.steps
            for _ in range(n):
                run(key, True)
    for v in res.values():
        v["wall_ms"], v["gpu_ms"] = _stats(v["wall_ms"]), _stats(v["gpu_ms"])
    for p in ("host", "device"):
        t, f = res[f"{p}_torch"], res[f"{p}_fused"]
        res[f"{p}_speedup_wall_median"] = round(t["wall_ms"]["median"] / f["wall_ms"]["median"], 3)
    return res


def kernel_rates(spec, dev, args):
    numels = spec.numels()
    shapes = [s for _, s in spec.params()]
    elems = sum(numels)
    k = HipKernels()
    tree = PackedTree(numels)
    inner = [t.view(s) for t, s in zip(synth.outer_tree_device(spec, dev), shapes)]
    tree.bind(SLOT_INNER, inner, torch.cuda.current_stream().cuda_stream)
    z = dict(dtype=torch.float32, device=dev)
    theta, wire, mom, m1, m2 = (torch.zeros(tree.total, **z) for _ in range(5))
    k.gather(tree, _lib.ALL_BUCKETS, SLOT_INNER, theta)
    flat = [p.view(-1) for p in inner]
    ms = {"dl_delta_pack_adamw": [], "dl_delta_pack_sgd": []}

    def launch(name, step):
        if name == "dl_delta_pack_adamw":
            k.delta_pack_adamw(tree, _lib.ALL_BUCKETS, SLOT_INNER, theta, wire, m1, m2,
                               adamw_scalars(CFG.lr, *CFG.betas, CFG.weight_decay, 1e-8,
                                             float(step)))
        else:
            k.delta_pack_sgd(tree, _lib.ALL_BUCKETS, SLOT_INNER, theta, wire, mom, 0.7, 0.9,
                             True, step == 1)

    for i in range(1, args.kernel_launches + 4):
        for name in (list(ms) if i % 2 else list(ms)[::-1]):
            synth.inner_tree_device(flat, i, 0, out=flat)  # after a launch inner == θ
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch(name, i)
            e1.record()
            torch.cuda.synchronize()
            if i > 3:  # the first launches load the code objects (and the SGD's first-step body)
                ms[name].append(e0.elapsed_time(e1))
    out = {"elements": elems}
    for name, bpp in (("dl_delta_pack_adamw", 36), ("dl_delta_pack_sgd", 28)):
        med = statistics.median(ms[name])
        out[name] = {"bytes_per_param": bpp, "ms": _stats(ms[name]),
                     "gbps_median": round(elems * bpp / (med * 1e-3) / 1e9, 1),
                     "fraction_of_8TBps": round(elems * bpp / (med * 1e-3) / HBM_PEAK, 4)}
    out["adamw_over_sgd_fraction"] = round(out["dl_delta_pack_adamw"]["fraction_of_8TBps"]
                                           / out["dl_delta_pack_sgd"]["fraction_of_8TBps"], 4)
    tree.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--torch-host-steps", type=int, default=2,
                    help="timed steps per round of the stock host path (seconds each on T125)")
    ap.add_argument("--kernel-launches", type=int, default=30)
    ap.add_argument("--tree", default="t125")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adamw_outer_bench measures on the GPU; no HIP device")
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", init_method="file://" + tempfile.mktemp(prefix="dlpg"),
                            rank=0, world_size=1)
    spec = get_tree(args.tree)
    out = {"tool": "tools/adamw_outer_bench.py", "tree": args.tree, "peers": 1,
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "args": {k: v for k, v in vars(args).items() if k != "out"},  # where it is written
           "optimizer": vars(CFG),                                        # is not a parameter
           "outer_step": outer_steps(spec, dev, args),
           "kernels": kernel_rates(spec, dev, args)}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
