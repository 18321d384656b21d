#!/usr/bin/env python3
"""The top-k wire's kernels (k = 64) beside their fp4 counterparts, direct launches on one GPU.

Each variant is one launch over the whole tree (DL_ALL_BUCKETS), inner bound; the pairs:
  dl_delta_topk              8.09 B/param   |  dl_delta_fp4              8.53
  dl_delta_topk + residual  16.09           |  dl_delta_fp4 + residual  16.53
  dl_topk_reduce (+ residual)  two peers' copies of half the tree's slots -> averaged slots
                                            |  dl_fp4_reduce (+ residual)
  dl_unpack_sgd_topk        20.09           |  dl_unpack_sgd_fp4        20.53
  dl_unpack_adamw_topk      28.09           |  dl_unpack_adamw_fp4      28.53

Method: tools/fp4_wire_bench.py's (its _measure: the variants alternate, their order rotated by
one every round; two untimed rounds; a 1 GiB copy through other memory before every timed
launch; device events; medians and each variant's own max - min), in a fresh child process
under its own time limit.

The bar, per pair: the HBM bytes are the fp4 kernel's to within 3 %, so the top-k kernel's median
should not exceed the fp4 counterpart's median by more than that counterpart's own max - min
over the rounds. A pair that misses is reported as missing, with the ratio; nothing is tuned
here.

--values fp4: the top-k wire's 4-bit-value kernels (dl_delta_topk_fp4, dl_topk_fp4_reduce,
dl_unpack_*_topk_fp4; 16 + 2k-byte slots) beside their exact-value counterparts above instead,
same method; the bar is the same with the exact-value kernel as the counterpart (the traffic is
the same to within 0.06 B/param).

    python tools/topk_wire_bench.py [--tree t125] [--rounds 9] [--out profiles/topk_wire_t125.json]
    python tools/topk_wire_bench.py --values fp4 --out profiles/topk_fp4_wire_t125.json
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

TOPK = 64
STEP_TIMEOUT_S = 300
PAIRS = (("dl_delta_topk", "dl_delta_fp4"), ("dl_delta_topk_residual", "dl_delta_fp4_residual"),
         ("dl_topk_reduce", "dl_fp4_reduce"), ("dl_topk_reduce_residual", "dl_fp4_reduce_residual"),
         ("dl_unpack_sgd_topk", "dl_unpack_sgd_fp4"), ("dl_unpack_adamw_topk", "dl_unpack_adamw_fp4"))
# --values fp4: the same six with the 4-bit-value kernel first and the exact-value one as counterpart
FP4_PAIRS = tuple((a.replace("topk", "topk_fp4"), a) for a, _ in PAIRS)


def step_kernels(args):
    import torch

    from diloco_amd import _lib
    from diloco_amd.kernels import FP4_SLOT, HipKernels, adamw_scalars
    from diloco_amd.plan import SLOT_INNER, PackedTree
    from diloco_amd.trees import get_tree
    from fp4_wire_bench import _measure

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
    inner = [(theta[o:o + n] - delta[o:o + n]).clone() for o, n in zip(offs, numels)]
    tree.bind(SLOT_INNER, inner, torch.cuda.current_stream().cuda_stream)
    resid = torch.zeros(tree.total, **z)
    mom = torch.randn(tree.total, generator=gen, **z) * 1e-2
    m1 = torch.randn(tree.total, generator=gen, **z) * 1e-2
    m2 = torch.rand(tree.total, generator=gen, **z) * 1e-4
    adam = adamw_scalars(0.01, 0.9, 0.95, 0.1, 1e-8, 2)
    m = -(-tree.n_chunks // 2)  # the reduce of one of two peers
    resid2 = torch.zeros(m * C, **z)
    sgd = (0.7, 0.9, True, False, SLOT_INNER)
    runs = {}
    pairs = FP4_PAIRS if args.values == "fp4" else PAIRS
    other = ("topk_fp4", _lib.TOPK_FP4_SLOT_BYTES(TOPK)) if args.values == "fp4" else ("fp4", FP4_SLOT)
    for tag, S in (("topk", _lib.TOPK_SLOT_BYTES(TOPK)), other):
        slots = torch.zeros(tree.n_chunks * S, dtype=torch.uint8, device=dev)
        if tag != "fp4":  # the two top-k kernel sets take the same arguments
            f = {n: getattr(k, n.replace("topk", tag)) for n in
                 ("delta_topk", "topk_reduce", "unpack_sgd_topk", "unpack_adamw_topk")}
            enc = lambda r, s=slots, f=f: f["delta_topk"](tree, all_, SLOT_INNER, theta, r, TOPK, s)  # noqa: E731
            red_ = lambda r, a, o, f=f: f["topk_reduce"](a, 2, m, 2, r, TOPK, o)  # noqa: E731
            usgd = lambda a, f=f: f["unpack_sgd_topk"](tree, all_, a, TOPK, theta, mom, *sgd)  # noqa: E731
            uadam = lambda a, f=f: f["unpack_adamw_topk"](tree, all_, a, TOPK, theta, m1, m2, adam,  # noqa: E731
                                                          SLOT_INNER)
        else:
            enc = lambda r, s=slots: k.delta_fp4(tree, all_, SLOT_INNER, theta, r, s)  # noqa: E731
            red_ = lambda r, a, o: k.fp4_reduce(a, 2, m, 2, r, o)  # noqa: E731
            usgd = lambda a: k.unpack_sgd_fp4(tree, all_, a, theta, mom, *sgd)  # noqa: E731
            uadam = lambda a: k.unpack_adamw_fp4(tree, all_, a, theta, m1, m2, adam, SLOT_INNER)  # noqa: E731
        enc(None)
        recv = torch.cat([slots[:m * S], slots[:m * S]]).contiguous()
        avg = slots.clone()  # the unpack kernels' input, never rewritten
        red = torch.zeros(m * S, dtype=torch.uint8, device=dev)
        wire, rbytes = tree.n_chunks * S, 3 * m * S
        runs.update({
            f"dl_delta_{tag}": (lambda f=enc: f(None), wire + 8 * elems),
            f"dl_delta_{tag}_residual": (lambda f=enc: f(resid), wire + 16 * elems),
            f"dl_{tag}_reduce": (lambda f=red_, a=recv, o=red: f(None, a, o), rbytes),
            f"dl_{tag}_reduce_residual": (lambda f=red_, a=recv, o=red: f(resid2, a, o),
                                          rbytes + 8 * m * C),
            f"dl_unpack_sgd_{tag}": (lambda f=usgd, a=avg: f(a), wire + 20 * elems),
            f"dl_unpack_adamw_{tag}": (lambda f=uadam, a=avg: f(a), wire + 28 * elems)})
    order = [n for pair in pairs for n in pair]  # counterparts are neighbours in a round
    res = _measure({n: runs[n] for n in order}, args.rounds)
    tree.close()
    return {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "k": TOPK,
            "elements": elems, "chunks": tree.n_chunks, "reduce_slots": m, "kernels": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--tree", default="t125")
    ap.add_argument("--values", choices=("f32", "fp4"), default="f32",
                    help="fp4: the 4-bit-value kernels beside the exact-value ones")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-out", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step_out:  # the child: the measurement, its result to the file the parent named
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("topk_wire_bench measures on the GPU; no HIP device")
        with open(args.step_out, "w") as f:
            json.dump(step_kernels(args), f)
        return
    part = os.path.join(tempfile.mkdtemp(prefix="dl_topk_bench_"), "kernels.json")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", args.tree,
                    "--rounds", str(args.rounds), "--values", args.values, "--step-out", part],
                   check=True, timeout=STEP_TIMEOUT_S)
    with open(part) as f:
        res = json.load(f)
    kn, bar = res["kernels"], {}
    for new, old in (FP4_PAIRS if args.values == "fp4" else PAIRS):
        a, b = kn[new], kn[old]
        bar[new] = {"counterpart": old, "median_ms": a["median_ms"],
                    "counterpart_median_ms": b["median_ms"],
                    "counterpart_max_minus_min_ms": b["max_minus_min_ms"],
                    "ratio": round(a["median_ms"] / b["median_ms"], 4),
                    "tbps": a["tbps_median"], "counterpart_tbps": b["tbps_median"],
                    "meets_bar": bool(a["median_ms"] <= b["median_ms"] + b["max_minus_min_ms"])}
    out = {"tool": "tools/topk_wire_bench.py", "tree": args.tree, "rounds": args.rounds,
           "cold": "a 1 GiB copy through other memory before every timed launch",
           "values": args.values,
           "bar": "median <= the counterpart's median + the counterpart's own max - min, same run "
                  "(counterpart: the fp4 wire's kernel; --values fp4: the exact-value top-k kernel)",
           "not_measured": ["any multi-GPU run", "any rate of the outer step at N > 1",
                            "the effect of k or of the sparse wire on a training run's loss"],
           **res, "pairs": bar, "all_meet_bar": all(v["meets_bar"] for v in bar.values())}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
