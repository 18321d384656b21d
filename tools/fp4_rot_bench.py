#!/usr/bin/env python3
"""The rotated fp4 wire's kernels beside the plain fp4 kernels, direct launches on one GPU.

Each variant is one launch over the whole tree (DL_ALL_BUCKETS), inner bound; the pairs move the
same algorithmic bytes:
  dl_delta_fp4_rot              |  dl_delta_fp4               8.53 B/param
  dl_delta_fp4_rot + residual   |  dl_delta_fp4 + residual   16.53
  dl_unpack_sgd_fp4_rot         |  dl_unpack_sgd_fp4         20.53 (steady step, inner written)
  dl_unpack_adamw_fp4_rot       |  dl_unpack_adamw_fp4       28.53
and dl_decode_fp4_rot (4.53 B/param) stands alone.

Method: tools/fp4_wire_bench.py's (_measure): the variants alternate pair by pair, the order
rotated by one every round; two untimed rounds, then --rounds timed ones; a 1 GiB copy through
other memory before every timed launch; device events; medians and each variant's own
max - min. The measurement runs in a fresh child process under its own time limit.

The bar, per pair: the rotated kernel's median does not exceed the plain kernel's median by more
than the plain kernel's own max - min over the rounds. A pair that misses is reported as
missing; nothing is tuned here.

    python tools/fp4_rot_bench.py [--tree t125] [--rounds 9] [--out profiles/fp4_rot_t125.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

from fp4_wire_bench import STEP_TIMEOUT_S, _measure

PAIRS = (("dl_delta_fp4_rot", "dl_delta_fp4"),
         ("dl_delta_fp4_rot_residual", "dl_delta_fp4_residual"),
         ("dl_unpack_sgd_fp4_rot", "dl_unpack_sgd_fp4"),
         ("dl_unpack_adamw_fp4_rot", "dl_unpack_adamw_fp4"))
SEED = 0x5EED


def step_kernels(args):
    import torch

    from diloco_amd import _lib
    from diloco_amd.kernels import FP4_SLOT, HipKernels, adamw_scalars
    from diloco_amd.plan import SLOT_INNER, PackedTree
    from diloco_amd.trees import get_tree

    dev = torch.device("cuda", 0)
    k = HipKernels()
    numels = get_tree(args.tree).numels()
    tree = PackedTree(numels)
    elems, A = sum(numels), _lib.ALL_BUCKETS
    gen = torch.Generator(device=dev).manual_seed(1)
    z = dict(dtype=torch.float32, device=dev)
    theta = torch.randn(tree.total, generator=gen, **z)
    delta = torch.randn(tree.total, generator=gen, **z) * 1e-2
    offs = [int(o) for o in tree.seg_off[:-1]]
    inner = [(theta[o:o + n] - delta[o:o + n]).clone() for o, n in zip(offs, numels)]
    tree.bind(SLOT_INNER, inner, torch.cuda.current_stream().cuda_stream)
    resid = torch.zeros(tree.total, **z)
    mom = torch.randn(tree.total, generator=gen, **z) * 1e-2
    m1 = torch.randn(tree.total, generator=gen, **z) * 1e-2
    m2 = torch.rand(tree.total, generator=gen, **z) * 1e-4
    dst = torch.zeros(tree.total, **z)
    adam = adamw_scalars(0.01, 0.9, 0.95, 0.1, 1e-8, 2)
    slots = torch.zeros(tree.n_chunks * FP4_SLOT, dtype=torch.uint8, device=dev)
    k.delta_fp4(tree, A, SLOT_INNER, theta, None, slots)
    avg = slots.clone()  # the steps' input, never rewritten
    wire = tree.n_chunks * FP4_SLOT
    sgd = (theta, mom, 0.7, 0.9, True, False, SLOT_INNER)
    runs = {
        "dl_delta_fp4_rot": (lambda: k.delta_fp4_rot(tree, A, SLOT_INNER, theta, None, SEED, slots),
                             wire + 8 * elems),
        "dl_delta_fp4": (lambda: k.delta_fp4(tree, A, SLOT_INNER, theta, None, slots),
                         wire + 8 * elems),
        "dl_delta_fp4_rot_residual": (lambda: k.delta_fp4_rot(tree, A, SLOT_INNER, theta, resid,
                                                              SEED, slots), wire + 16 * elems),
        "dl_delta_fp4_residual": (lambda: k.delta_fp4(tree, A, SLOT_INNER, theta, resid, slots),
                                  wire + 16 * elems),
        "dl_unpack_sgd_fp4_rot": (lambda: k.unpack_sgd_fp4_rot(tree, A, avg, SEED, *sgd),
                                  wire + 20 * elems),
        "dl_unpack_sgd_fp4": (lambda: k.unpack_sgd_fp4(tree, A, avg, *sgd), wire + 20 * elems),
        "dl_unpack_adamw_fp4_rot": (lambda: k.unpack_adamw_fp4_rot(
            tree, A, avg, SEED, theta, m1, m2, adam, SLOT_INNER), wire + 28 * elems),
        "dl_unpack_adamw_fp4": (lambda: k.unpack_adamw_fp4(
            tree, A, avg, theta, m1, m2, adam, SLOT_INNER), wire + 28 * elems),
        "dl_decode_fp4_rot": (lambda: k.decode_fp4_rot(tree, A, avg, SEED, dst), wire + 4 * elems),
    }
    res = _measure(runs, args.rounds)
    tree.close()
    return {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
            "elements": elems, "chunks": tree.n_chunks, "kernels": res}


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
            raise SystemExit("fp4_rot_bench measures on the GPU; no HIP device")
        with open(args.step_out, "w") as f:
            json.dump(step_kernels(args), f)
        return
    part = os.path.join(tempfile.mkdtemp(prefix="dl_fp4_rot_bench_"), "kernels.json")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", args.tree,
                    "--rounds", str(args.rounds), "--step-out", part],
                   check=True, timeout=STEP_TIMEOUT_S)
    with open(part) as f:
        res = json.load(f)
    kn, bar = res["kernels"], {}
    for new, old in PAIRS:
        a, b = kn[new], kn[old]
        bar[new] = {"counterpart": old, "median_ms": a["median_ms"],
                    "counterpart_median_ms": b["median_ms"],
                    "counterpart_max_minus_min_ms": b["max_minus_min_ms"],
                    "tbps": a["tbps_median"], "counterpart_tbps": b["tbps_median"],
                    "meets_bar": bool(a["median_ms"] <= b["median_ms"] + b["max_minus_min_ms"])}
    out = {"tool": "tools/fp4_rot_bench.py", "tree": args.tree, "rounds": args.rounds,
           "cold": "a 1 GiB copy through other memory before every timed launch",
           "bar": "median <= the plain fp4 kernel's median + that kernel's own max - min, same run",
           "not_measured": ["any multi-GPU run", "any rate of the outer step at N > 1",
                            "the effect of the rotation on a training run's loss"],
           **res, "pairs": bar}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
