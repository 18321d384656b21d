"""The outer step on the gathered top-k slots on one GPU: dl_unpack_sgd_topk_ag and
dl_unpack_adamw_topk_ag in their two accumulate forms (per-peer barriers; wave-owned quarters,
tuning build only) at n = 2 and n = 8 peers, beside the pair each replaces on one rank --
dl_topk_reduce over the rank's 1/n share of the slots (no residual) plus dl_unpack_sgd_topk /
dl_unpack_adamw_topk over the whole tree -- and beside that fused decoder alone (the same dense
traffic, one slot per chunk instead of n).

Method (tools/topk_ag_bench.py's): tree T125, k = 64, whole-tree direct launches timed with
events, a 512-MiB write between launches so every launch starts cold, every variant alternated in
one run with the order rotated every round, two untimed rounds then nine timed, medians with min
and max. SGD is the steady-state Nesterov step (momentum loaded and stored), both rules write the
inner model. The bar per rule and n: the new kernel's median is not above the pair's summed
medians plus the pair's own max - min (summed).
Needs the tuning build: make -C diloco-swarm_amd/csrc TUNING=1 and DILOCO_HIP_LIB=<that file>."""
import argparse
import json
import statistics

import torch

from diloco_amd import _lib
from diloco_amd.kernels import HipKernels, adamw_scalars
from diloco_amd.plan import SLOT_INNER
from diloco_amd.trees import get_tree
from topk_ag_bench import K_ENTRIES, ROUNDS, WARM, slots

PEERS = (2, 8)
SGD = (0.7, 0.9, True, False)
ADAM = adamw_scalars(0.01, 0.9, 0.95, 0.1, 1e-8, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.load()
    if not lib.dl_tuning_build():
        raise SystemExit("the wave-owned form exists in the tuning build only")
    dev, K, ALL = torch.device("cuda:0"), HipKernels(), _lib.ALL_BUCKETS
    numels = get_tree("t125").numels()
    tree = K.tree(numels, dev)
    nch = tree.n_chunks
    inner = [torch.zeros(n, device=dev) for n in numels]  # alive for as long as they are bound
    K.bind(tree, SLOT_INNER, inner, dev)
    th, m1 = torch.randn(tree.total, device=dev), torch.randn(tree.total, device=dev) * 1e-3
    m2 = torch.rand(tree.total, device=dev) * 1e-6
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    data = {n: slots(n, nch, dev) for n in (1,) + PEERS}
    share = {n: -(-nch // n) for n in PEERS}
    recv = {n: slots(n, share[n], dev) for n in PEERS}
    red = torch.zeros(share[2] * 6 * K_ENTRIES, dtype=torch.uint8, device=dev)

    def ag(rule, form, n):
        def run():
            lib.dl_tune_topk_ag_form(form)
            if rule == "sgd":
                K.unpack_sgd_topk_ag(tree, ALL, data[n], n, nch, K_ENTRIES, th, m1, *SGD, SLOT_INNER)
            else:
                K.unpack_adamw_topk_ag(tree, ALL, data[n], n, nch, K_ENTRIES, th, m1, m2, ADAM, SLOT_INNER)
        return run

    variants = {
        "dl_unpack_sgd_topk": lambda: K.unpack_sgd_topk(tree, ALL, data[1], K_ENTRIES, th, m1, *SGD, SLOT_INNER),
        "dl_unpack_adamw_topk": lambda: K.unpack_adamw_topk(tree, ALL, data[1], K_ENTRIES, th, m1, m2, ADAM,
                                                            SLOT_INNER),
    }
    for n in PEERS:
        variants[f"dl_topk_reduce_share_n{n}"] = (
            lambda n=n: K.topk_reduce(recv[n], n, share[n], n, None, K_ENTRIES, red))
        for rule in ("sgd", "adamw"):
            variants[f"{rule}_ag_barriers_n{n}"] = ag(rule, 0, n)
            variants[f"{rule}_ag_waves_n{n}"] = ag(rule, 1, n)

    names, times = list(variants), {v: [] for v in variants}
    for rnd in range(WARM + ROUNDS):
        for name in names[rnd % len(names):] + names[:rnd % len(names)]:
            flush.fill_(rnd & 0xFF)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            variants[name]()
            b.record()
            b.synchronize()
            if rnd >= WARM:
                times[name].append(a.elapsed_time(b) * 1e3)
    lib.dl_tune_topk_ag_form(0)
    v = {name: {"median": statistics.median(t), "min": min(t), "max": max(t)} for name, t in times.items()}
    rec = {"tree": "t125", "params": sum(numels), "k": K_ENTRIES, "rounds": ROUNDS, "unit": "us",
           "variants": v, "bar": {}}
    for rule in ("sgd", "adamw"):
        for n in PEERS:
            pair = [v[f"dl_topk_reduce_share_n{n}"], v[f"dl_unpack_{rule}_topk"]]
            limit = sum(p["median"] + p["max"] - p["min"] for p in pair)
            rec["bar"][f"{rule}_n{n}"] = {
                "pair_summed_medians": sum(p["median"] for p in pair), "limit": limit,
                **{form: {"median": v[f"{rule}_ag_{form}_n{n}"]["median"],
                          "met": v[f"{rule}_ag_{form}_n{n}"]["median"] <= limit}
                   for form in ("barriers", "waves")}}
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    tree.close()


if __name__ == "__main__":
    main()
