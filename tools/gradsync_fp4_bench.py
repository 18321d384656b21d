#!/usr/bin/env python3
"""The fp4 gradient-sync kernels beside their int8 counterparts, direct launches on one GPU.

Each variant is one launch over the whole tree (DL_ALL_BUCKETS), gradients bound (one allocation
per tensor, as a model's are):
  dl_gather_fp4 (no residual)   4.53 B/param   g read; slots written        | dl_gather_q8       5.02
  dl_gather_fp4 (residual)     12.53 B/param   g, r read; slots, r written  | dl_gather_q8_ef   13.02
  dl_unpack_avg_fp4             4.53 B/param   slots read; .grad written    | dl_unpack_avg_q8   5.02
  dl_unpack_avg_fp4 (partials)  the same with the per-chunk Σ g²            | the same with partials

Method, as tools/gradsync_q8_bench.py: the variants alternate, their order rotated by one every
round; two untimed rounds, then --rounds timed ones; a 1 GiB copy through other memory before
every timed launch; device events on the launch stream; medians and each variant's own max - min.
The measurement runs in a fresh child process under its own time limit. No time is fixed in
advance: the yardstick of each fp4 kernel is its int8 counterpart in the same run -- it moves
fewer bytes, so it should not be slower -- and the margin is the counterpart's own max - min.

    python tools/gradsync_fp4_bench.py [--tree t125] [--rounds 9] [--out profiles/gradsync_fp4_t125.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "diloco-swarm_amd"))
sys.path.insert(0, os.path.join(HERE, "tools"))

from q8_ef_bench import _measure  # noqa: E402  (the alternated, rotated, cold timing loop)

STEP_TIMEOUT_S = 240
# fp4 kernel -> its int8 counterpart
COUNTERPART = {"dl_gather_fp4": "dl_gather_q8", "dl_gather_fp4_residual": "dl_gather_q8_ef",
               "dl_unpack_avg_fp4": "dl_unpack_avg_q8",
               "dl_unpack_avg_fp4_partials": "dl_unpack_avg_q8_partials"}
# fp32 B/param moved besides the slots
F32_BYTES = {"dl_gather_fp4": 4, "dl_gather_fp4_residual": 12, "dl_unpack_avg_fp4": 4,
             "dl_unpack_avg_fp4_partials": 4}


def step_kernels(args):
    import torch

    from diloco_amd import _lib
    from diloco_amd.kernels import FP4_SLOT, Q8_SLOT, HipKernels
    from diloco_amd.plan import SLOT_GRAD, PackedTree
    from diloco_amd.trees import get_tree

    dev = torch.device("cuda", 0)
    k = HipKernels()
    numels = get_tree(args.tree).numels()
    tree = PackedTree(numels)
    elems, all_ = sum(numels), _lib.ALL_BUCKETS
    gen = torch.Generator(device=dev).manual_seed(1)
    z = dict(dtype=torch.float32, device=dev)
    grads = [torch.randn(n, generator=gen, **z) * 1e-2 for n in numels]
    tree.bind(SLOT_GRAD, grads, torch.cuda.current_stream().cuda_stream)
    resid = {w: torch.zeros(tree.total, **z) for w in ("fp4", "q8")}
    u8 = dict(dtype=torch.uint8, device=dev)
    slots = {"fp4": torch.zeros(tree.n_chunks * FP4_SLOT, **u8),
             "q8": torch.zeros(tree.n_chunks * Q8_SLOT, **u8)}
    # the decoders' inputs: valid slots no encoder rewrites
    avg = {w: torch.zeros_like(s) for w, s in slots.items()}
    k.gather_fp4(tree, all_, SLOT_GRAD, None, avg["fp4"])
    k.gather_q8(tree, all_, SLOT_GRAD, avg["q8"])
    partials = torch.zeros(tree.n_chunks, dtype=torch.float64, device=dev)
    launches = {
        "dl_gather_fp4": lambda: k.gather_fp4(tree, all_, SLOT_GRAD, None, slots["fp4"]),
        "dl_gather_q8": lambda: k.gather_q8(tree, all_, SLOT_GRAD, slots["q8"]),
        "dl_gather_fp4_residual": lambda: k.gather_fp4(tree, all_, SLOT_GRAD, resid["fp4"],
                                                       slots["fp4"]),
        "dl_gather_q8_ef": lambda: k.gather_q8_ef(tree, all_, SLOT_GRAD, resid["q8"], slots["q8"]),
        "dl_unpack_avg_fp4": lambda: k.unpack_avg_fp4(tree, all_, avg["fp4"], SLOT_GRAD),
        "dl_unpack_avg_q8": lambda: k.unpack_avg_q8(tree, all_, avg["q8"], SLOT_GRAD),
        "dl_unpack_avg_fp4_partials": lambda: k.unpack_avg_fp4(tree, all_, avg["fp4"], SLOT_GRAD,
                                                               partials),
        "dl_unpack_avg_q8_partials": lambda: k.unpack_avg_q8(tree, all_, avg["q8"], SLOT_GRAD,
                                                             partials),
    }
    nbytes = {}
    for f, q in COUNTERPART.items():
        nbytes[f] = F32_BYTES[f] * elems + tree.n_chunks * FP4_SLOT
        nbytes[q] = F32_BYTES[f] * elems + tree.n_chunks * Q8_SLOT
    res = _measure({name: (fn, nbytes[name]) for name, fn in launches.items()}, args.rounds)
    tree.close()
    return {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
            "elements": elems, "chunks": tree.n_chunks, "bytes": nbytes, "kernels": res}


def summarise(res, args):
    """Each fp4 kernel against its int8 counterpart of the same run."""
    kn, compare = res["kernels"], {}
    for f, q in COUNTERPART.items():
        margin = kn[q]["max_minus_min_ms"]
        compare[f] = {"counterpart": q, "median_ms": kn[f]["median_ms"],
                      "counterpart_median_ms": kn[q]["median_ms"],
                      "counterpart_max_minus_min_ms": margin,
                      "bytes_per_param": round(res["bytes"][f] / res["elements"], 3),
                      "counterpart_bytes_per_param": round(res["bytes"][q] / res["elements"], 3),
                      "not_slower_within_the_counterparts_spread":
                          bool(kn[f]["median_ms"] <= kn[q]["median_ms"] + margin)}
    return {"tool": "tools/gradsync_fp4_bench.py", "tree": args.tree, "rounds": args.rounds,
            "cold": "a 1 GiB copy through other memory before every timed launch",
            "not_measured": ["any run on more than one GPU", "any rate at N > 1",
                             "the effect on a training run's loss"],
            **res, "against_int8": compare}


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
            raise SystemExit("gradsync_fp4_bench measures on the GPU; no HIP device")
        with open(args.step_out, "w") as f:
            json.dump(step_kernels(args), f)
        return
    part = os.path.join(tempfile.mkdtemp(prefix="dl_gradsync_fp4_bench_"), "kernels.json")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", args.tree, "--rounds",
                    str(args.rounds), "--step-out", part], check=True, timeout=STEP_TIMEOUT_S)
    with open(part) as f:
        res = json.load(f)
    text = json.dumps(summarise(res, args), indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
