#!/usr/bin/env python3
"""The int8 gradient-sync kernels beside their neighbours, direct launches on one GPU.

Step "kernels", each variant one launch over the whole tree (DL_ALL_BUCKETS), gradients bound
(one allocation per tensor, as a model's are):
  dl_gather            8 B/param      g read; the fp32 wire written
  dl_gather_q8         5.02 B/param   g read; slots written
  dl_gather_q8_ef     13.02 B/param   g, residual read; slots and residual written
  dl_delta_q8          9.02 B/param   θ, inner read; slots written (the encoders' sibling)
  dl_unpack_avg        8 B/param      the fp32 wire read (/ 2); .grad written (the decoder's sibling)
  dl_unpack_avg_sumsq  8 B/param      the same with the per-chunk Σ g²
  dl_unpack_avg_q8     5.02 B/param   slots read; .grad written; with and without partials
Step "probes": the dl_copy read and write probes over 1 and 2 equal streams, each stream the size
of the tree, for the same-run ceiling of a kernel's byte mix,
t >= R / BW_read(s_r) + W / BW_write(s_w), the 1 KB-per-chunk payload counted as a stream.

Method, as tools/q8_ef_bench.py: the variants alternate, their order rotated by one every round;
two untimed rounds, then --rounds timed ones; a 1 GiB copy through other memory before every
timed launch; device events on the launch stream; medians and each variant's own max - min.
Every step runs in a fresh child process under its own time limit, and a step that fails ends
the run. No rate is claimed in advance: the result reports every kernel's fraction of its own
ceiling, and for each new kernel whether its fraction is lower than its sibling's (dl_delta_q8
for the encoders, dl_unpack_avg for the decoder) by more than the sibling's own
(max - min) / median.

    python tools/gradsync_q8_bench.py [--tree t125] [--rounds 9] [--out profiles/gradsync_q8_t125.json]
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
STEPS = ("kernels", "probes")
# kernel -> fp32 B/param read and written, the streams of each side, and whether the slots
# (1.016 B/param) are among the bytes written or read
MIX = {
    "dl_gather": dict(read=4, rs=1, write=4, ws=1),
    "dl_gather_q8": dict(read=4, rs=1, write=0, ws=1, q8_written=True),
    "dl_gather_q8_ef": dict(read=8, rs=2, write=4, ws=2, q8_written=True),
    "dl_delta_q8": dict(read=8, rs=2, write=0, ws=1, q8_written=True),
    "dl_unpack_avg": dict(read=4, rs=1, write=4, ws=1),
    "dl_unpack_avg_sumsq": dict(read=4, rs=1, write=4, ws=1),
    "dl_unpack_avg_q8": dict(read=0, rs=1, write=4, ws=1, q8_read=True),
    "dl_unpack_avg_q8_partials": dict(read=0, rs=1, write=4, ws=1, q8_read=True),
}
SIBLING = {"dl_gather_q8": "dl_delta_q8", "dl_gather_q8_ef": "dl_delta_q8",
           "dl_unpack_avg_q8": "dl_unpack_avg", "dl_unpack_avg_q8_partials": "dl_unpack_avg"}


def _bytes(name, elems, q8):
    m = MIX[name]
    r = m["read"] * elems + (q8 if m.get("q8_read") else 0)
    w = m["write"] * elems + (q8 if m.get("q8_written") else 0)
    return r, w


def step_kernels(args):
    import torch

    from diloco_amd import _lib
    from diloco_amd.kernels import Q8_SLOT, HipKernels
    from diloco_amd.plan import SLOT_GRAD, SLOT_INNER, PackedTree
    from diloco_amd.trees import get_tree

    dev = torch.device("cuda", 0)
    k = HipKernels()
    numels = get_tree(args.tree).numels()
    tree = PackedTree(numels)
    elems, all_ = sum(numels), _lib.ALL_BUCKETS
    gen = torch.Generator(device=dev).manual_seed(1)
    z = dict(dtype=torch.float32, device=dev)
    theta = torch.randn(tree.total, generator=gen, **z)
    offs = [int(o) for o in tree.seg_off[:-1]]
    inner = [theta[o:o + n].clone() * 0.99 for o, n in zip(offs, numels)]
    grads = [torch.randn(n, generator=gen, **z) * 1e-2 for n in numels]
    stream = torch.cuda.current_stream().cuda_stream
    tree.bind(SLOT_INNER, inner, stream)
    tree.bind(SLOT_GRAD, grads, stream)
    wire = torch.randn(tree.total, generator=gen, **z)
    resid = torch.zeros(tree.total, **z)
    slots = torch.zeros(tree.n_chunks * Q8_SLOT, dtype=torch.uint8, device=dev)
    avg = torch.zeros_like(slots)  # the decoder's input: valid slots no encoder rewrites
    k.gather_q8(tree, all_, SLOT_GRAD, avg)
    partials = torch.zeros(tree.n_chunks, dtype=torch.float64, device=dev)
    q8 = tree.n_chunks * Q8_SLOT
    launches = {
        "dl_gather": lambda: k.gather(tree, all_, SLOT_GRAD, wire),
        "dl_gather_q8": lambda: k.gather_q8(tree, all_, SLOT_GRAD, slots),
        "dl_gather_q8_ef": lambda: k.gather_q8_ef(tree, all_, SLOT_GRAD, resid, slots),
        "dl_delta_q8": lambda: k.delta_q8(tree, all_, SLOT_INNER, theta, slots),
        "dl_unpack_avg": lambda: k.unpack_avg(tree, all_, wire, 2, SLOT_GRAD),
        "dl_unpack_avg_sumsq": lambda: k.unpack_avg_sumsq(tree, all_, wire, 2, SLOT_GRAD,
                                                          partials),
        "dl_unpack_avg_q8": lambda: k.unpack_avg_q8(tree, all_, avg, SLOT_GRAD),
        "dl_unpack_avg_q8_partials": lambda: k.unpack_avg_q8(tree, all_, avg, SLOT_GRAD,
                                                             partials),
    }
    runs = {name: (fn, sum(_bytes(name, elems, q8))) for name, fn in launches.items()}
    res = _measure(runs, args.rounds)
    tree.close()
    return {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
            "elements": elems, "chunks": tree.n_chunks, "slot_bytes": q8, "kernels": res}


def step_probes(args):
    import torch

    from diloco_amd import _lib
    from diloco_amd.trees import get_tree

    elems = sum(get_tree(args.tree).numels())
    stream = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(2 * elems + 64, dtype=torch.float32, device="cuda:0")

    def probe(kind, s):
        nbytes = 4 * s * elems // (16 * s) * (16 * s)  # s equal streams of whole float4s
        flags = _lib.TUNE_NT_LOADS | kind | _lib.COPY_STREAMS(s)
        src, dst = ((buf.data_ptr(), None) if kind == _lib.COPY_READ else (None, buf.data_ptr()))
        return (lambda: _lib.call("dl_copy", src, dst, nbytes, flags, stream), nbytes)

    runs = {"read_probe_1": probe(_lib.COPY_READ, 1), "read_probe_2": probe(_lib.COPY_READ, 2),
            "write_probe_1": probe(_lib.COPY_WRITE, 1), "write_probe_2": probe(_lib.COPY_WRITE, 2)}
    return {"probes": _measure(runs, args.rounds)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--tree", default="t125")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=STEPS, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--step-out", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:  # a child: one step, its result to the file the parent named
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("gradsync_q8_bench measures on the GPU; no HIP device")
        res = {"kernels": step_kernels, "probes": step_probes}[args.step](args)
        with open(args.step_out, "w") as f:
            json.dump(res, f)
        return
    res, tmp = {}, tempfile.mkdtemp(prefix="dl_gradsync_q8_bench_")
    for step in STEPS:  # fresh processes, each under its own limit; a failure ends the run
        part = os.path.join(tmp, step + ".json")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", args.tree,
                        "--rounds", str(args.rounds), "--step", step, "--step-out", part],
                       check=True, timeout=STEP_TIMEOUT_S)
        with open(part) as f:
            res.update(json.load(f))
    text = json.dumps(summarise(res, args), indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


def summarise(res, args):
    """The ceilings, fractions and sibling comparisons from one run's kernels and probes."""
    kn, elems, q8 = res["kernels"], res["elements"], res["slot_bytes"]
    ceiling = {"formula": "t >= R / BW_read(s_r) + W / BW_write(s_w), same-run dl_copy probes"}
    for name, m in MIX.items():
        r, w = _bytes(name, elems, q8)
        bw_r = res["probes"][f"read_probe_{m['rs']}"]["gbps_median"] * 1e9
        bw_w = res["probes"][f"write_probe_{m['ws']}"]["gbps_median"] * 1e9
        ms = (r / bw_r + w / bw_w) * 1e3
        ceiling[name] = {"read_bytes": r, "write_bytes": w, "read_streams": m["rs"],
                         "write_streams": m["ws"], "ceiling_ms": round(ms, 5),
                         "fraction_of_ceiling": round(ms / kn[name]["median_ms"], 4),
                         "spread_over_median": round(kn[name]["max_minus_min_ms"]
                                                     / kn[name]["median_ms"], 4)}
    compare = {}
    for name, sib in SIBLING.items():
        f, fs = ceiling[name]["fraction_of_ceiling"], ceiling[sib]["fraction_of_ceiling"]
        margin = fs * ceiling[sib]["spread_over_median"]  # the sibling's own spread
        compare[name] = {"sibling": sib, "fraction": f, "sibling_fraction": fs,
                         "sibling_margin": round(margin, 4),
                         "below_sibling_by_more_than_its_spread": bool(fs - f > margin)}
    return {"tool": "tools/gradsync_q8_bench.py", "tree": args.tree, "rounds": args.rounds,
            "cold": "a 1 GiB copy through other memory before every timed launch",
            "not_measured": ["any run on more than one GPU", "any rate at N > 1",
                             "the effect on a training run's loss"],
            **res, "ceiling": ceiling, "against_sibling": compare}


if __name__ == "__main__":
    main()
