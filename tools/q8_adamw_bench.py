#!/usr/bin/env python3
"""dl_unpack_adamw_q8 beside its neighbours, direct launches over a whole tree on one GPU.

Variants, each one launch over the whole tree (DL_ALL_BUCKETS) with the inner params bound:
  dl_unpack_adamw_q8   29.02 B/param  the averaged int8 slots, AdamW, inner write
  dl_unpack_sgd_q8     21.02 B/param  the same slots, Nesterov SGD (steady step), inner write
  dl_unpack_adamw      32 B/param     fp32 wire, divisor 2, AdamW, inner write
  dl_unpack_sgd        24 B/param     fp32 wire, divisor 2, Nesterov SGD, inner write
  dl_copy              8 B/param      the flat NT copy of the same number of elements
The slots are what dl_delta_q8 writes for θ - inner of random data, so every chunk has a real
scale. Method: the variants alternate, their order rotated by one every round; two untimed
rounds, then --rounds timed ones; a 1 GiB copy through other memory before every timed launch
(the operands leave the Infinity Cache); device events on the launch stream; medians and each
variant's own max - min. GB/s is over the bytes the algorithm needs.

The claim it checks (no parent-commit counterpart exists: the kernel is new): the new kernel's
median is not above dl_unpack_adamw's by more than dl_unpack_adamw's own max - min, and its
GB/s relative to dl_unpack_adamw sits where dl_unpack_sgd_q8's does relative to dl_unpack_sgd.

    python tools/q8_adamw_bench.py [--tree t125] [--rounds 9] [--out FILE]

--rehearse N instead times the reference's four calls on the int8 wire with N gloo processes on
the ONE GPU (a gloo rehearsal: the collectives are staged through the host, so it says what the
step costs beside the same exchange, not what a multi-GPU run would): OuterAdamW fused
(dl_unpack_adamw_q8), OuterAdamW eager (DILOCO_OUTER_FUSED=0: decode, then dl_unpack_adamw) and
stock torch.optim.AdamW on the fused outer model (torch's own step body on the decoded .grad:
what OuterAdamW fell back to on this wire before dl_unpack_adamw_q8 existed), both placements,
alternated; host clock around the four calls ending in a device synchronise, per rank.
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "diloco-swarm_amd"))

import torch  # noqa: E402

from diloco_amd import _lib  # noqa: E402
from diloco_amd.kernels import Q8_SLOT, HipKernels, adamw_scalars  # noqa: E402
from diloco_amd.plan import SLOT_INNER, PackedTree  # noqa: E402
from diloco_amd.trees import get_tree  # noqa: E402

HBM_PEAK = 8e12  # B/s
FLUSH_BYTES = 1 << 30
ALL = _lib.ALL_BUCKETS


def _stats(ms, nbytes):
    med = statistics.median(ms)
    return {"ms": [round(x, 5) for x in ms], "median_ms": round(med, 5),
            "max_minus_min_ms": round(max(ms) - min(ms), 5), "bytes": nbytes,
            "gbps_median": round(nbytes / (med * 1e-3) / 1e9, 1),
            "fraction_of_8TBps": round(nbytes / (med * 1e-3) / HBM_PEAK, 4)}


def _rehearse_worker(rank, world, port, args, out):
    import time
    from types import SimpleNamespace

    import torch.distributed as dist

    os.environ.update(DILOCO_DP_BACKEND="gloo", RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    for v in ("DILOCO_OUTER_EXCHANGE", "DILOCO_DP_EXCHANGE", "DILOCO_OUTER_WIRE"):
        os.environ.pop(v, None)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank,
                            world_size=world)
    from diloco_amd import synth
    from diloco_amd.comm import TrainingComm
    from diloco_amd.utils import (compute_pseudo_gradient, get_optimizer, get_outer_model,
                                  sync_inner_model)
    from diloco_amd.world import World

    dev = torch.device("cuda", 0)
    spec = get_tree(args.tree)
    shapes = [s for _, s in spec.params()]
    cfg = SimpleNamespace(type="AdamW", lr=0.01, weight_decay=0.1, betas=(0.9, 0.95))
    comm = TrainingComm(World.from_default_group(1), (1, 1, spec.n_embd), None)
    setups = {}
    for placement in ("host", "device"):
        for variant in ("fused", "eager", "torch"):
            inner = torch.nn.Module()
            inner.ps = torch.nn.ParameterList([torch.nn.Parameter(t.view(s)) for t, s in zip(
                synth.outer_tree_device(spec, dev), shapes)])
            outer = get_outer_model(inner, "device" if placement == "device" else None,
                                    fused=variant != "eager", wire="int8")
            if variant == "torch":
                os.environ.pop("DILOCO_OUTER_ADAMW", None)
            else:
                os.environ["DILOCO_OUTER_ADAMW"] = "fused"
            setups[placement, variant] = (inner, outer, get_optimizer(outer, cfg), [0])
    ms = {k: [] for k in setups}

    def run(key, timed):
        inner, outer, opt, count = setups[key]
        count[0] += 1
        flat = [p.data.view(-1) for p in inner.parameters()]
        synth.inner_tree_device(flat, count[0], rank, out=flat)  # nonzero, rank-specific deltas
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        compute_pseudo_gradient(inner, outer)
        comm.sync_gradients(outer)
        opt.step()
        sync_inner_model(outer, inner)
        torch.cuda.synchronize()
        if timed:
            ms[key].append((time.perf_counter() - t0) * 1e3)

    keys = list(setups)
    for r in range(args.rounds + 2):
        for key in keys[r % len(keys):] + keys[:r % len(keys)]:
            run(key, r >= 2)
    res = {"_".join(k): {"optimizer": type(setups[k][2]).__name__,
                         "wall_ms": [round(x, 3) for x in v],
                         "median_ms": round(statistics.median(v), 3),
                         "max_minus_min_ms": round(max(v) - min(v), 3)} for k, v in ms.items()}
    with open(os.path.join(out, f"r{rank}.json"), "w") as f:
        json.dump(res, f)
    dist.barrier()
    dist.destroy_process_group()


def rehearse(args):
    import socket
    import tempfile

    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = tempfile.mkdtemp(prefix="dl_q8_adamw_")
    mp.spawn(_rehearse_worker, args=(args.rehearse, port, args, out), nprocs=args.rehearse,
             join=True)
    ranks = []
    for r in range(args.rehearse):
        with open(os.path.join(out, f"r{r}.json")) as f:
            ranks.append(json.load(f))
    return {"tool": "tools/q8_adamw_bench.py --rehearse", "tree": args.tree,
            "label": "gloo rehearsal: N processes on ONE GPU, collectives staged through the "
                     "host; not a multi-GPU run and not a rate",
            "peers": args.rehearse, "wire": "int8", "rounds": args.rounds,
            "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
            "what": "host clock around the reference's four calls ending in a device "
                    "synchronise, per rank; variants alternated, order rotated every round",
            "ranks": ranks}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--tree", default="t125")
    ap.add_argument("--out", default=None)
    ap.add_argument("--rehearse", type=int, default=0, metavar="N",
                    help="time the four calls over N gloo processes on the one GPU instead")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("q8_adamw_bench measures on the GPU; no HIP device")
    if args.rehearse:
        text = json.dumps(rehearse(args), indent=1)
        print(text)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    dev = torch.device("cuda", 0)
    k = HipKernels()
    spec = get_tree(args.tree)
    numels = spec.numels()
    tree = PackedTree(numels)
    elems = sum(numels)
    gen = torch.Generator(device=dev).manual_seed(1)
    z = dict(dtype=torch.float32, device=dev)
    theta = torch.randn(tree.total, generator=gen, **z)
    wire = torch.randn(tree.total, generator=gen, **z) * 1e-2
    m1, m2, mom, dst = (torch.zeros(tree.total, **z) for _ in range(4))
    # the inner params: one allocation per tensor, as a model's are
    offs = [int(o) for o in tree.seg_off[:-1]]
    inner = [(theta[o:o + n] + wire[o:o + n]).clone() for o, n in zip(offs, numels)]
    stream = torch.cuda.current_stream().cuda_stream
    tree.bind(SLOT_INNER, inner, stream)
    slots = torch.zeros(tree.n_chunks * Q8_SLOT, dtype=torch.uint8, device=dev)
    k.delta_q8(tree, ALL, SLOT_INNER, theta, slots)
    flush_a = torch.zeros(FLUSH_BYTES // 4, **z)
    flush_b = torch.empty_like(flush_a)
    step = [0]

    def sc():
        step[0] += 1  # AdamW's bias corrections move with the step count, as in a run
        return adamw_scalars(0.01, 0.9, 0.95, 0.1, 1e-8, float(step[0]))

    q8_bytes = tree.n_chunks * Q8_SLOT
    runs = {  # name -> (launch, algorithmic bytes)
        "dl_unpack_adamw_q8": (
            lambda: k.unpack_adamw_q8(tree, ALL, slots, theta, m1, m2, sc(), SLOT_INNER),
            q8_bytes + 28 * elems),
        "dl_unpack_sgd_q8": (
            lambda: k.unpack_sgd_q8(tree, ALL, slots, theta, mom, 0.7, 0.9, True, False,
                                    SLOT_INNER), q8_bytes + 20 * elems),
        "dl_unpack_adamw": (
            lambda: k.unpack_adamw(tree, ALL, wire, 2, theta, m1, m2, sc(), SLOT_INNER),
            32 * elems),
        "dl_unpack_sgd": (
            lambda: k.unpack_sgd(tree, ALL, wire, 2, theta, mom, 0.7, 0.9, True, False,
                                 SLOT_INNER), 24 * elems),
        "dl_copy": (
            lambda: _lib.call("dl_copy", wire.data_ptr(), dst.data_ptr(), 4 * (elems // 4 * 4),
                              _lib.TUNE_NT_LOADS, stream), 8 * (elems // 4 * 4)),
    }
    ms = {name: [] for name in runs}
    names = list(runs)
    for r in range(args.rounds + 2):
        order = names[r % len(names):] + names[:r % len(names)]
        for name in order:
            flush_b.copy_(flush_a)  # the operands leave the Infinity Cache
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            runs[name][0]()
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:  # the first two rounds load the code objects
                ms[name].append(e0.elapsed_time(e1))
    res = {name: _stats(ms[name], runs[name][1]) for name in runs}
    new, ada = res["dl_unpack_adamw_q8"], res["dl_unpack_adamw"]
    sq8, sgd = res["dl_unpack_sgd_q8"], res["dl_unpack_sgd"]
    out = {"tool": "tools/q8_adamw_bench.py", "tree": args.tree,
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "rounds": args.rounds, "elements": elems, "chunks": tree.n_chunks,
           "cold": "a 1 GiB copy through other memory before every timed launch",
           "not_measured": ["a multi-GPU run", "any rate of the outer step at N > 1"],
           "kernels": res,
           "claim": {
               "adamw_q8_minus_adamw_median_ms": round(new["median_ms"] - ada["median_ms"], 5),
               "adamw_own_max_minus_min_ms": ada["max_minus_min_ms"],
               "not_slower_than_adamw_within_its_spread":
                   new["median_ms"] - ada["median_ms"] <= ada["max_minus_min_ms"],
               "adamw_q8_over_adamw_gbps": round(new["gbps_median"] / ada["gbps_median"], 4),
               "sgd_q8_over_sgd_gbps": round(sq8["gbps_median"] / sgd["gbps_median"], 4)}}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    tree.close()


if __name__ == "__main__":
    main()
