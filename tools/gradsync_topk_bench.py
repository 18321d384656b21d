#!/usr/bin/env python3
"""The top-k gradient-sync kernels beside their counterparts, direct launches on one GPU.

Each variant is one launch over the whole tree (DL_ALL_BUCKETS) at k = --topk, gradients bound (one
allocation per tensor, as a model's are), for both value formats (slot = 6k or 16 + 2k bytes):
  dl_gather_topk[_fp4] (no residual)   4 B/param + slots   | dl_delta_topk[_fp4]             8 + slots
  dl_gather_topk[_fp4] (residual)     12 B/param + slots   | dl_delta_topk[_fp4] (residual) 16 + slots
  dl_unpack_avg_topk[_fp4]             4 B/param + slots   | dl_unpack_avg_fp4               4.53
  dl_unpack_avg_topk[_fp4] (partials)  the same with the per-chunk Σ g²  | the same with partials

Method, as tools/gradsync_fp4_bench.py (its _measure loop): the variants alternate, their order
rotated by one every round; two untimed rounds, then --rounds timed ones; a 1 GiB copy through
other memory before every timed launch; device events on the launch stream; medians and each
variant's own max - min. The measurement runs in a fresh child process under its own time limit.
No time is fixed in advance: an encoder reads 4 B/param less than the outer step's and runs the
same selection, a decoder writes the fp4 decoder's 4 B/param and reads fewer slot bytes, so
neither should be slower; the margin is the counterpart's own max - min.

    python tools/gradsync_topk_bench.py [--tree t125] [--topk 64] [--rounds 9] [--out profiles/gradsync_topk_t125.json]
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

STEP_TIMEOUT_S = 300
SFX = {"f32": "", "fp4": "_fp4"}


def counterparts():
    """new kernel -> (its counterpart, fp32 B/param of the new kernel, of the counterpart)."""
    out = {}
    for s in SFX.values():
        out[f"dl_gather_topk{s}"] = (f"dl_delta_topk{s}", 4, 8)
        out[f"dl_gather_topk{s}_residual"] = (f"dl_delta_topk{s}_residual", 12, 16)
        out[f"dl_unpack_avg_topk{s}"] = ("dl_unpack_avg_fp4", 4, 4)
        out[f"dl_unpack_avg_topk{s}_partials"] = ("dl_unpack_avg_fp4_partials", 4, 4)
    return out


def step_kernels(args):
    import torch

    from diloco_amd import _lib
    from diloco_amd.gradsync import slot_wire_bytes
    from diloco_amd.kernels import FP4_SLOT, HipKernels
    from diloco_amd.plan import SLOT_GRAD, SLOT_INNER, PackedTree
    from diloco_amd.trees import get_tree

    dev = torch.device("cuda", 0)
    k, kk = HipKernels(), args.topk
    numels = get_tree(args.tree).numels()
    tree = PackedTree(numels)
    elems, all_, nch = sum(numels), _lib.ALL_BUCKETS, tree.n_chunks
    gen = torch.Generator(device=dev).manual_seed(1)
    z = dict(dtype=torch.float32, device=dev)
    u8 = dict(dtype=torch.uint8, device=dev)
    grads = [torch.randn(n, generator=gen, **z) * 1e-2 for n in numels]
    stream = torch.cuda.current_stream().cuda_stream
    tree.bind(SLOT_GRAD, grads, stream)
    # the outer step's encoder: θ packed, inner bound; θ - inner has the gradients' distribution
    tree.bind(SLOT_INNER, [torch.zeros(n, **z) for n in numels], stream)
    theta = torch.randn(tree.total, generator=gen, **z) * 1e-2
    partials = torch.zeros(nch, dtype=torch.float64, device=dev)
    fp4_avg = torch.zeros(nch * FP4_SLOT, **u8)  # the decoders' inputs: valid slots nothing rewrites
    k.gather_fp4(tree, all_, SLOT_GRAD, None, fp4_avg)
    launches = {
        "dl_unpack_avg_fp4": lambda: k.unpack_avg_fp4(tree, all_, fp4_avg, SLOT_GRAD),
        "dl_unpack_avg_fp4_partials": lambda: k.unpack_avg_fp4(tree, all_, fp4_avg, SLOT_GRAD,
                                                               partials)}
    slot_bytes = {"dl_unpack_avg_fp4": FP4_SLOT, "dl_unpack_avg_fp4_partials": FP4_SLOT}

    def add(values, s):
        S = slot_wire_bytes("topk", kk, values)
        gather, delta = getattr(k, "gather_topk" + s), getattr(k, "delta_topk" + s)
        unpack = getattr(k, "unpack_avg_topk" + s)
        slots, avg = torch.zeros(nch * S, **u8), torch.zeros(nch * S, **u8)
        r_g, r_d = torch.zeros(tree.total, **z), torch.zeros(tree.total, **z)
        gather(tree, all_, SLOT_GRAD, None, kk, avg)
        new = {
            f"dl_gather_topk{s}": lambda: gather(tree, all_, SLOT_GRAD, None, kk, slots),
            f"dl_delta_topk{s}": lambda: delta(tree, all_, SLOT_INNER, theta, None, kk, slots),
            f"dl_gather_topk{s}_residual": lambda: gather(tree, all_, SLOT_GRAD, r_g, kk, slots),
            f"dl_delta_topk{s}_residual": lambda: delta(tree, all_, SLOT_INNER, theta, r_d, kk, slots),
            f"dl_unpack_avg_topk{s}": lambda: unpack(tree, all_, avg, kk, SLOT_GRAD),
            f"dl_unpack_avg_topk{s}_partials": lambda: unpack(tree, all_, avg, kk, SLOT_GRAD,
                                                              partials)}
        launches.update(new)
        slot_bytes.update({name: S for name in new})

    for values, s in SFX.items():
        add(values, s)
    nbytes = {}
    for new, (old, f_new, f_old) in counterparts().items():
        nbytes[new] = f_new * elems + nch * slot_bytes[new]
        nbytes[old] = f_old * elems + nch * slot_bytes[old]
    res = _measure({name: (fn, nbytes[name]) for name, fn in launches.items()}, args.rounds)
    tree.close()
    return {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
            "elements": elems, "chunks": nch, "bytes": nbytes, "kernels": res}


def summarise(res, args):
    """Each new kernel against its counterpart of the same run."""
    kn, compare = res["kernels"], {}
    for new, (old, _f_new, _f_old) in counterparts().items():
        margin = kn[old]["max_minus_min_ms"]
        compare[new] = {"counterpart": old, "median_ms": kn[new]["median_ms"],
                        "max_minus_min_ms": kn[new]["max_minus_min_ms"],
                        "counterpart_median_ms": kn[old]["median_ms"],
                        "counterpart_max_minus_min_ms": margin,
                        "bytes_per_param": round(res["bytes"][new] / res["elements"], 3),
                        "counterpart_bytes_per_param": round(res["bytes"][old] / res["elements"], 3),
                        "not_slower_within_the_counterparts_spread":
                            bool(kn[new]["median_ms"] <= kn[old]["median_ms"] + margin)}
    return {"tool": "tools/gradsync_topk_bench.py", "tree": args.tree, "topk": args.topk,
            "rounds": args.rounds,
            "cold": "a 1 GiB copy through other memory before every timed launch",
            "not_measured": ["any run on more than one GPU", "any rate at N > 1",
                             "the effect on a training run's loss"],
            **res, "against_counterparts": compare}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--tree", default="t125")
    ap.add_argument("--topk", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-out", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step_out:  # the child: the measurement, its result to the file the parent named
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("gradsync_topk_bench measures on the GPU; no HIP device")
        with open(args.step_out, "w") as f:
            json.dump(step_kernels(args), f)
        return
    part = os.path.join(tempfile.mkdtemp(prefix="dl_gradsync_topk_bench_"), "kernels.json")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", args.tree, "--topk",
                    str(args.topk), "--rounds", str(args.rounds), "--step-out", part], check=True,
                   timeout=STEP_TIMEOUT_S)
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
