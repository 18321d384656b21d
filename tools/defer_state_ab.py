#!/usr/bin/env python3
"""Same-process A/B of DILOCO_OUTER_DEFER_STATE on the bench headline (the reference's four
calls at one peer, the default outer model): two outer models built side by side in one
process, the switch on for one and off for the other, timed in alternating blocks of K steps
with the order rotated every round. Allocation placement moves this kernel by several per cent
between fresh processes; here both variants keep their allocations for the whole
run, so the rounds differ by the switch alone.

    python tools/defer_state_ab.py [--tree t125] [--steps 20] [--rounds 6]

One JSON object on stdout: every block's ms per step, and the medians.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "diloco-swarm_amd"))

SWITCH = "DILOCO_OUTER_DEFER_STATE"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default="t125")
    ap.add_argument("--steps", type=int, default=20, help="steps per block (even)")
    ap.add_argument("--rounds", type=int, default=6)
    a = ap.parse_args()

    import torch

    import bench
    from diloco_amd.trees import get_tree
    from diloco_amd.utils import compute_pseudo_gradient, sync_inner_model

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    spec = get_tree(a.tree)

    def build(on):
        os.environ[SWITCH] = "1" if on else "0"
        inner, outer, opt, comm = bench._dropin_objects(spec, dev, 0, "f32", None, None)
        assert outer._diloco_mirror.dev.defer_state == on

        def one():
            compute_pseudo_gradient(inner, outer)
            comm.sync_gradients(outer)
            opt.step()
            sync_inner_model(outer, inner)
        return one, outer

    runs = {"on": build(True), "off": build(False)}

    def block(one):
        for _ in range(2):
            one()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(a.steps):
            one()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / a.steps

    ms = {"on": [], "off": []}
    order = []
    for r in range(a.rounds):
        names = ("on", "off") if r % 2 == 0 else ("off", "on")
        order.append("-".join(names))
        for n in names:
            ms[n].append(round(block(runs[n][0]), 5))
    med = {n: statistics.median(v) for n, v in ms.items()}
    P = spec.total()
    print(json.dumps({"tree": spec.name, "params": P, "steps_per_block": a.steps, "order": order,
                      "ms_per_step": ms, "median_ms": med,
                      "median_GBs_4P": {n: round(4.0 * P / (v * 1e-3) / 1e9, 1)
                                        for n, v in med.items()},
                      "on_over_off": round(med["on"] / med["off"], 4)}))
    for _, outer in runs.values():
        outer._diloco_mirror.close()


if __name__ == "__main__":
    main()
