#!/usr/bin/env python3
"""Gradient-norm clipping on ONE GPU: diloco_amd.utils.clip_grad_norm_ and the fused
GradSync.sync(max_norm) beside torch.nn.utils.clip_grad_norm_ (the reference's call,
src/train.py:255) on the same synthetic device gradients, in one process.

Variants, alternated with the order rotated every round; each timed call sits between two
device events on the launch stream, after a 1 GiB copy through other memory and a synchronise,
so it starts with the Infinity Cache holding none of its operands. Two untimed rounds load the
code objects. Every sample is kept.

    torch_clip            torch's call, max_norm above the norm (it still rewrites every grad)
    hip_clip_no_clip      utils.clip_grad_norm_, max_norm above the norm: one read, 4 B/param
    hip_clip_clipping     utils.clip_grad_norm_, max_norm at half the norm: 12 B/param
    torch_clip_clipping   torch's call, max_norm at half the norm
    sync_then_torch_clip  GradSync.sync() (one replica) then torch's call, not clipping
    sync_fused            GradSync.sync(max_norm), not clipping

Before a clipping call the gradients are doubled (untimed), so every such call scales by about
one half. The claim the profile supports or retracts: hip_clip_no_clip's median lies below
torch_clip's by more than torch_clip's own round-to-round spread (max - min).

Not measured here: more than one replica (the collectives), a model's real gradients.

    python tools/clip_norm_bench.py [--tree t125] [--rounds 9] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "diloco-swarm_amd"))

import torch  # noqa: E402

from diloco_amd import utils  # noqa: E402
from diloco_amd.gradsync import GradSync  # noqa: E402
from diloco_amd.trees import get_tree  # noqa: E402

FLUSH_BYTES = 1 << 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default="t125")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_norm_bench measures on the GPU; no HIP device")
    dev = torch.device("cuda", 0)
    spec = get_tree(args.tree)
    numels = spec.numels()
    elems = sum(numels)
    gen = torch.Generator(device=dev).manual_seed(1)
    params = []
    for n in numels:
        p = torch.nn.Parameter(torch.empty(n, device=dev))
        p.grad = torch.randn(n, generator=gen, device=dev, dtype=torch.float32) * 1e-2
        params.append(p)
    grads = [p.grad for p in params]
    gs = GradSync(params, None, 1)
    flush_a = torch.zeros(FLUSH_BYTES // 4, device=dev)
    flush_b = torch.empty_like(flush_a)
    norm0 = float(utils.clip_grad_norm_(params, float("inf")))
    big, half = 1e30, norm0 / 2

    def double():
        torch._foreach_mul_(grads, 2.0)

    tclip = torch.nn.utils.clip_grad_norm_
    runs = {  # name -> (untimed preparation or None, timed call)
        "torch_clip": (None, lambda: tclip(params, big)),
        "hip_clip_no_clip": (None, lambda: utils.clip_grad_norm_(params, big)),
        "hip_clip_clipping": (double, lambda: utils.clip_grad_norm_(params, half)),
        "torch_clip_clipping": (double, lambda: tclip(params, half)),
        "sync_then_torch_clip": (None, lambda: (gs.sync(), tclip(params, big))),
        "sync_fused": (None, lambda: gs.sync(big)),
    }
    utils.clip_grad_norm_(params, half)  # the clipping variants start from norm == half
    ms = {name: [] for name in runs}
    names = list(runs)
    for r in range(args.rounds + 2):
        order = names[r % len(names):] + names[:r % len(names)]
        for name in order:
            prep, call = runs[name]
            if prep is not None:
                prep()
            flush_b.copy_(flush_a)  # the operands leave the Infinity Cache
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:  # the first two rounds load the code objects
                ms[name].append(e0.elapsed_time(e1))
    res = {}
    for name, v in ms.items():
        med = statistics.median(v)
        res[name] = {"ms": [round(x, 5) for x in v], "median_ms": round(med, 5),
                     "min_ms": round(min(v), 5), "max_ms": round(max(v), 5),
                     "spread_ms": round(max(v) - min(v), 5)}
    res["hip_clip_no_clip"]["gbps_of_4B_per_param"] = round(
        4 * elems / (res["hip_clip_no_clip"]["median_ms"] * 1e-3) / 1e9, 1)
    t, h = res["torch_clip"], res["hip_clip_no_clip"]
    gap = t["median_ms"] - h["median_ms"]
    out = {"tool": "tools/clip_norm_bench.py", "tree": args.tree, "elements": elems,
           "tensors": len(numels), "device": torch.cuda.get_device_name(0),
           "torch": torch.__version__, "rounds": args.rounds, "norm": norm0,
           "cold": "a 1 GiB copy through other memory before every timed call",
           "timing": "device events on the launch stream around the whole call",
           "not_measured": ["more than one replica", "a model's real gradients"],
           "variants": res,
           "claim": {"statement": "hip_clip_no_clip median below torch_clip median by more than "
                                  "torch_clip's own spread (max - min)",
                     "median_gap_ms": round(gap, 5), "torch_spread_ms": t["spread_ms"],
                     "holds": bool(gap > t["spread_ms"])},
           "fused_sync_saving_ms": round(res["sync_then_torch_clip"]["median_ms"]
                                         - res["sync_fused"]["median_ms"], 5)}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    gs.close()


if __name__ == "__main__":
    main()
