#!/usr/bin/env python3
"""The fp4 wire's kernels beside their int8 counterparts, direct launches on one GPU.

Each variant is one launch over the whole tree (DL_ALL_BUCKETS), inner bound; the pairs:
  dl_delta_fp4              8.53 B/param   |  dl_delta_q8          9.02
  dl_delta_fp4 + residual  16.53           |  dl_delta_q8_ef      17.02
  dl_fp4_reduce             two peers' copies of half the tree's slots -> averaged slots,
                            3 x 0.531 B per owned param   |  dl_q8_reduce  3 x 1.016
  dl_fp4_reduce + residual  + 8 B          |  dl_q8_reduce_ef
  dl_unpack_sgd_fp4        20.53 (steady step: θ, momentum read and written, inner written)
                                           |  dl_unpack_sgd_q8    21.02
  dl_unpack_adamw_fp4      28.53           |  dl_unpack_adamw_q8  29.02

Method, as tools/q8_ef_bench.py: the variants alternate, their order rotated by one every round;
two untimed rounds, then --rounds timed ones; a 1 GiB copy through other memory before every
timed launch; device events on the launch stream; medians and each variant's own max - min. The
measurement runs in a fresh child process under its own time limit.

The bar, per pair: the fp4 kernel moves fewer algorithmic bytes, and its median does not exceed
the int8 counterpart's median by more than that counterpart's own max - min over the rounds. A
pair that misses is reported as missing; nothing is tuned here. Each kernel's TB/s over its
algorithmic bytes stands beside its counterpart's from the same run.

    python tools/fp4_wire_bench.py [--tree t125] [--rounds 9] [--out profiles/fp4_wire_t125.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "diloco-swarm_amd"))

FLUSH_BYTES = 1 << 30
STEP_TIMEOUT_S = 300
PAIRS = (("dl_delta_fp4", "dl_delta_q8"), ("dl_delta_fp4_residual", "dl_delta_q8_ef"),
         ("dl_fp4_reduce", "dl_q8_reduce"), ("dl_fp4_reduce_residual", "dl_q8_reduce_ef"),
         ("dl_unpack_sgd_fp4", "dl_unpack_sgd_q8"), ("dl_unpack_adamw_fp4", "dl_unpack_adamw_q8"))


def _stats(ms, nbytes):
    med = statistics.median(ms)
    return {"ms": [round(x, 5) for x in ms], "median_ms": round(med, 5),
            "max_minus_min_ms": round(max(ms) - min(ms), 5), "bytes": nbytes,
            "tbps_median": round(nbytes / (med * 1e-3) / 1e12, 4)}


def _measure(runs, rounds):
    """runs: name -> (launch, algorithmic bytes). Alternated, rotated, cold, device events."""
    import torch

    z = dict(dtype=torch.float32, device="cuda:0")
    flush_a = torch.zeros(FLUSH_BYTES // 4, **z)
    flush_b = torch.empty_like(flush_a)
    ms = {name: [] for name in runs}
    names = list(runs)
    for r in range(rounds + 2):
        for name in names[r % len(names):] + names[:r % len(names)]:
            flush_b.copy_(flush_a)  # the operands leave the Infinity Cache
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            runs[name][0]()
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:  # the first two rounds load the code objects
                ms[name].append(e0.elapsed_time(e1))
    return {name: _stats(ms[name], runs[name][1]) for name in runs}


def step_kernels(args):
    import torch

    from diloco_amd import _lib
    from diloco_amd.kernels import FP4_SLOT, Q8_SLOT, HipKernels, adamw_scalars
    from diloco_amd.plan import SLOT_INNER, PackedTree
    from diloco_amd.trees import get_tree

    dev = torch.device("cuda", 0)
    k = HipKernels()
    numels = get_tree(args.tree).numels()
    tree = PackedTree(numels)
    elems, all_, C = sum(numels), _lib.ALL_BUCKETS, _lib.CHUNK_ELEMS
    gen = torch.Generator(device=dev).manual_seed(1)
    z = dict(dtype=torch.float32, device=dev)
    theta = torch.randn(tree.total, generator=gen, **z)
    delta = torch.randn(tree.total, generator=gen, **z) * 1e-2
    offs = [int(o) for o in tree.seg_off[:-1]]
    # the inner params: one allocation per tensor, as a model's are
    inner = [(theta[o:o + n] - delta[o:o + n]).clone() for o, n in zip(offs, numels)]
    tree.bind(SLOT_INNER, inner, torch.cuda.current_stream().cuda_stream)
    resid = torch.zeros(tree.total, **z)
    mom = torch.randn(tree.total, generator=gen, **z) * 1e-2
    m1 = torch.randn(tree.total, generator=gen, **z) * 1e-2
    m2 = torch.rand(tree.total, generator=gen, **z) * 1e-4
    adam = adamw_scalars(0.01, 0.9, 0.95, 0.1, 1e-8, 2)
    # the reduce of one of two peers: m = half the tree's slots from each of two ranks
    m = -(-tree.n_chunks // 2)
    resid2 = torch.zeros(m * C, **z)
    runs = {}
    for tag, S in (("fp4", FP4_SLOT), ("q8", Q8_SLOT)):
        slots = torch.zeros(tree.n_chunks * S, dtype=torch.uint8, device=dev)
        if tag == "fp4":
            k.delta_fp4(tree, all_, SLOT_INNER, theta, None, slots)
        else:
            k.delta_q8(tree, all_, SLOT_INNER, theta, slots)
        recv = torch.cat([slots[:m * S], slots[:m * S]]).contiguous()
        avg = slots.clone()  # the unpack kernels' input, never rewritten
        red = torch.zeros(m * S, dtype=torch.uint8, device=dev)
        wire, rbytes = tree.n_chunks * S, 3 * m * S
        if tag == "fp4":
            runs.update({
                "dl_delta_fp4": (lambda s=slots: k.delta_fp4(tree, all_, SLOT_INNER, theta, None, s),
                                 wire + 8 * elems),
                "dl_delta_fp4_residual": (lambda s=slots: k.delta_fp4(tree, all_, SLOT_INNER, theta,
                                                                       resid, s), wire + 16 * elems),
                "dl_fp4_reduce": (lambda r=recv, o=red: k.fp4_reduce(r, 2, m, 2, None, o), rbytes),
                "dl_fp4_reduce_residual": (lambda r=recv, o=red: k.fp4_reduce(r, 2, m, 2, resid2, o),
                                           rbytes + 8 * m * C),
                "dl_unpack_sgd_fp4": (lambda a=avg: k.unpack_sgd_fp4(
                    tree, all_, a, theta, mom, 0.7, 0.9, True, False, SLOT_INNER), wire + 20 * elems),
                "dl_unpack_adamw_fp4": (lambda a=avg: k.unpack_adamw_fp4(
                    tree, all_, a, theta, m1, m2, adam, SLOT_INNER), wire + 28 * elems)})
        else:
            runs.update({
                "dl_delta_q8": (lambda s=slots: k.delta_q8(tree, all_, SLOT_INNER, theta, s),
                                wire + 8 * elems),
                "dl_delta_q8_ef": (lambda s=slots: k.delta_q8_ef(tree, all_, SLOT_INNER, theta,
                                                                  resid, s), wire + 16 * elems),
                "dl_q8_reduce": (lambda r=recv, o=red: k.q8_reduce(r, 2, m, 2, o), rbytes),
                "dl_q8_reduce_ef": (lambda r=recv, o=red: k.q8_reduce_ef(r, 2, m, 2, resid2, o),
                                    rbytes + 8 * m * C),
                "dl_unpack_sgd_q8": (lambda a=avg: k.unpack_sgd_q8(
                    tree, all_, a, theta, mom, 0.7, 0.9, True, False, SLOT_INNER), wire + 20 * elems),
                "dl_unpack_adamw_q8": (lambda a=avg: k.unpack_adamw_q8(
                    tree, all_, a, theta, m1, m2, adam, SLOT_INNER), wire + 28 * elems)})
    # fp4 and int8 interleaved pair by pair, so neighbours in a round are counterparts
    order = [n for pair in PAIRS for n in pair]
    res = _measure({n: runs[n] for n in order}, args.rounds)
    tree.close()
    return {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
            "elements": elems, "chunks": tree.n_chunks, "reduce_slots": m, "kernels": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--tree", default="t125")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-out", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step_out:  # the child: the measurement, its result to the file the parent named
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("fp4_wire_bench measures on the GPU; no HIP device")
        with open(args.step_out, "w") as f:
            json.dump(step_kernels(args), f)
        return
    part = os.path.join(tempfile.mkdtemp(prefix="dl_fp4_bench_"), "kernels.json")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", args.tree,
                    "--rounds", str(args.rounds), "--step-out", part],
                   check=True, timeout=STEP_TIMEOUT_S)
    with open(part) as f:
        res = json.load(f)
    kn, bar = res["kernels"], {}
    for new, old in PAIRS:
        a, b = kn[new], kn[old]
        allowed = b["median_ms"] + b["max_minus_min_ms"]
        bar[new] = {"counterpart": old, "fewer_bytes": a["bytes"] < b["bytes"],
                    "median_ms": a["median_ms"], "counterpart_median_ms": b["median_ms"],
                    "counterpart_max_minus_min_ms": b["max_minus_min_ms"],
                    "tbps": a["tbps_median"], "counterpart_tbps": b["tbps_median"],
                    "meets_bar": bool(a["bytes"] < b["bytes"] and a["median_ms"] <= allowed)}
    out = {"tool": "tools/fp4_wire_bench.py", "tree": args.tree, "rounds": args.rounds,
           "cold": "a 1 GiB copy through other memory before every timed launch",
           "bar": "fewer algorithmic bytes than the int8 counterpart, and median <= the "
                  "counterpart's median + the counterpart's own max - min, same run",
           "not_measured": ["any multi-GPU run", "any rate of the outer step at N > 1",
                            "the effect of the 4-bit wire on a training run's loss"],
           **res, "pairs": bar, "all_meet_bar": all(v["meets_bar"] for v in bar.values())}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
