#!/usr/bin/env python3
"""The inner AdamW step on ONE GPU: optim.InnerAdamW (one dl_adamw_step pass, 28 B/param)
beside stock torch.optim.AdamW on device tensors (the reference's inner_optimizer.step(),
src/train.py:257; torch's _multi_tensor_adam, nine foreach passes), on synthetic device
parameters and gradients of a named tree, in one process.

Variants, alternated with the order rotated every round; each timed call sits between two
device events on the launch stream, after a 1 GiB copy through other memory and a synchronise,
so it starts with the Infinity Cache holding none of its operands. Two untimed rounds load the
code objects and create the optimizer state. Every sample is kept.

    torch_adamw            stock AdamW.step() on device tensors
    fused_adamw            InnerAdamW.step()
    clip_then_torch_adamw  utils.clip_grad_norm_ at half the norm (it clips), then stock AdamW
    fold_fused_adamw       InnerAdamW.clip_grad_norm_ at half the norm, then InnerAdamW.step():
                           the coefficient is applied inside the step, the gradients stay as
                           they are

Before a clip_then_torch_adamw call its gradients are doubled (untimed), so every such call
scales by about one half; the folded variant never changes its gradients. The two stock
variants share one model and optimizer, the two fused ones another. The claim the profile
supports or retracts: fused_adamw's median lies below torch_adamw's by more than torch_adamw's
own round-to-round spread (max - min).

Not measured here: more than one replica, a model's real gradients, the forward pass that
re-reads θ after the step (the step's θ stores are non-temporal).

    python tools/inner_adamw_bench.py [--tree t125] [--rounds 9] [--out FILE]
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
from diloco_amd.optim import InnerAdamW  # noqa: E402
from diloco_amd.trees import get_tree  # noqa: E402

FLUSH_BYTES = 1 << 30
HBM_PEAK = 8e12  # B/s
HYPER = dict(lr=6e-4, betas=(0.9, 0.95), weight_decay=0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default="t125")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rounds < 9:
        raise SystemExit("inner_adamw_bench: at least 9 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("inner_adamw_bench measures on the GPU; no HIP device")
    dev = torch.device("cuda", 0)
    spec = get_tree(args.tree)
    numels = spec.numels()
    elems = sum(numels)
    gen = torch.Generator(device=dev).manual_seed(1)

    def model():
        ps = []
        for n in numels:
            p = torch.nn.Parameter(torch.randn(n, generator=gen, device=dev) * 0.02)
            p.grad = torch.randn(n, generator=gen, device=dev, dtype=torch.float32) * 1e-2
            ps.append(p)
        return ps

    stock_p, fused_p = model(), model()
    stock = torch.optim.AdamW(stock_p, **HYPER)
    fused = InnerAdamW(fused_p, **HYPER)
    stock_g = [p.grad for p in stock_p]
    flush_a = torch.zeros(FLUSH_BYTES // 4, device=dev)
    flush_b = torch.empty_like(flush_a)
    half_stock = float(utils.clip_grad_norm_(stock_p, float("inf"))) / 2
    half_fused = float(utils.clip_grad_norm_(fused_p, float("inf"))) / 2

    def double():
        torch._foreach_mul_(stock_g, 2.0)

    def fold():
        fused.clip_grad_norm_(half_fused)
        fused.step()

    runs = {  # name -> (untimed preparation or None, timed call)
        "torch_adamw": (None, stock.step),
        "fused_adamw": (None, fused.step),
        "clip_then_torch_adamw": (double, lambda: (utils.clip_grad_norm_(stock_p, half_stock),
                                                   stock.step())),
        "fold_fused_adamw": (None, fold),
    }
    utils.clip_grad_norm_(stock_p, half_stock)  # the clipping variant starts from norm == half
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
            if r >= 2:  # the first two rounds load the code objects and create the state
                ms[name].append(e0.elapsed_time(e1))
    res = {}
    for name, v in ms.items():
        med = statistics.median(v)
        res[name] = {"ms": [round(x, 5) for x in v], "median_ms": round(med, 5),
                     "min_ms": round(min(v), 5), "max_ms": round(max(v), 5),
                     "spread_ms": round(max(v) - min(v), 5)}
    for name in ("fused_adamw", "torch_adamw"):
        rate = 28 * elems / (res[name]["median_ms"] * 1e-3)
        res[name]["gbps_of_28B_per_param"] = round(rate / 1e9, 1)
        res[name]["fraction_of_8TBps"] = round(rate / HBM_PEAK, 4)
    t, h = res["torch_adamw"], res["fused_adamw"]
    gap = t["median_ms"] - h["median_ms"]
    out = {"tool": "tools/inner_adamw_bench.py", "tree": args.tree, "elements": elems,
           "tensors": len(numels), "device": torch.cuda.get_device_name(0),
           "torch": torch.__version__, "rounds": args.rounds, "hyper": HYPER,
           "cold": "a 1 GiB copy through other memory before every timed call",
           "timing": "device events on the launch stream around the whole call",
           "not_measured": ["more than one replica", "a model's real gradients",
                            "the forward pass that re-reads theta after the step's "
                            "non-temporal stores"],
           "variants": res,
           "claim": {"statement": "fused_adamw median below torch_adamw median by more than "
                                  "torch_adamw's own spread (max - min)",
                     "median_gap_ms": round(gap, 5), "torch_spread_ms": t["spread_ms"],
                     "holds": bool(gap > t["spread_ms"])},
           "speedup_fused_over_torch": round(t["median_ms"] / h["median_ms"], 3),
           "fold_saving_ms": round(res["clip_then_torch_adamw"]["median_ms"]
                                   - res["fold_fused_adamw"]["median_ms"], 5)}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
