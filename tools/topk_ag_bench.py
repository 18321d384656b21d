"""The all-gather exchange's gradient decoder on one GPU: dl_unpack_avg_topk_ag in its two
accumulate forms (per-peer barriers, the product's; wave-owned quarters, tuning build only) at
n = 2 and n = 8 peers, beside the pair it replaces on one rank at n = 2: dl_topk_reduce over the
rank's 1/2 share of the slots (no residual) plus dl_unpack_avg_topk over the whole tree.

Method (tools/topk_wire_bench.py's): tree T125, k = 64, direct launches timed with events, a
512-MiB write between launches so every launch starts cold, the variants alternated with the
order rotated every round, two untimed rounds then nine timed, medians with min and max.
Needs the tuning build: make -C diloco-swarm_amd/csrc TUNING=1 and DILOCO_HIP_LIB=<that file>."""
import argparse
import json
import statistics

import torch

from diloco_amd import _lib
from diloco_amd.kernels import HipKernels
from diloco_amd.plan import SLOT_GRAD
from diloco_amd.trees import get_tree

K_ENTRIES, ROUNDS, WARM = 64, 9, 2


def slots(n, nch, dev):
    """[n][nch] valid 6k-byte slots: ascending distinct positions, small random values."""
    pos = (torch.arange(K_ENTRIES, device=dev) * (4096 // K_ENTRIES)
           + torch.randint(0, 4096 // K_ENTRIES, (n, nch, K_ENTRIES), device=dev)).to(torch.int16)
    val = torch.randn(n, nch, K_ENTRIES, device=dev) * 1e-3
    return torch.cat([val.view(torch.uint8).reshape(n, nch, -1),
                      pos.view(torch.uint8).reshape(n, nch, -1)], dim=2).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.load()
    if not lib.dl_tuning_build():
        raise SystemExit("the wave-owned form exists in the tuning build only")
    dev, K = torch.device("cuda:0"), HipKernels()
    numels = get_tree("t125").numels()
    tree = K.tree(numels, dev)
    nch, half = tree.n_chunks, -(-tree.n_chunks // 2)
    grads = [torch.zeros(n, device=dev) for n in numels]  # alive for as long as they are bound
    K.bind(tree, SLOT_GRAD, grads, dev)
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    data = {n: slots(n, nch, dev) for n in (1, 2, 8)}
    recv, red = slots(2, half, dev), torch.zeros(half * 6 * K_ENTRIES, dtype=torch.uint8, device=dev)

    def ag(form, n):
        def run():
            lib.dl_tune_topk_ag_form(form)
            K.unpack_avg_topk_ag(tree, _lib.ALL_BUCKETS, data[n], n, nch, K_ENTRIES, SLOT_GRAD)
        return run

    variants = {
        "dl_topk_reduce_half_n2": lambda: K.topk_reduce(recv, 2, half, 2, None, K_ENTRIES, red),
        "dl_unpack_avg_topk": lambda: K.unpack_avg_topk(tree, _lib.ALL_BUCKETS, data[1], K_ENTRIES,
                                                        SLOT_GRAD),
    }
    for n in (2, 8):
        variants[f"ag_barriers_n{n}"] = ag(0, n)
        variants[f"ag_waves_n{n}"] = ag(1, n)

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
    rec = {"tree": "t125", "params": sum(numels), "k": K_ENTRIES, "rounds": ROUNDS, "unit": "us",
           "variants": {v: {"median": statistics.median(t), "min": min(t), "max": max(t)}
                        for v, t in times.items()}}
    rec["pair_summed_medians_n2"] = (rec["variants"]["dl_topk_reduce_half_n2"]["median"]
                                     + rec["variants"]["dl_unpack_avg_topk"]["median"])
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    tree.close()


if __name__ == "__main__":
    main()
