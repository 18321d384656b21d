#!/usr/bin/env python3
"""The int8 wire's error-feedback kernels beside their neighbours, direct launches on one GPU.

Step "kernels", each variant one launch over the whole tree (DL_ALL_BUCKETS), inner bound:
  dl_delta_q8_ef    17.02 B/param  θ, inner, residual read; slots and residual written
  dl_delta_q8        9.02 B/param  θ, inner read; slots written
  dl_delta_pack     12 B/param     θ, inner read; the fp32 wire written
  dl_q8_reduce_ef   two peers' copies of half the tree's slots -> averaged slots, with the
                    owner's residual read and rewritten (2 x 4 B per value)
  dl_q8_reduce      the same without the residual
Step "probes": the dl_copy read probe over 3 and 2 equal streams and the write probe over 2 and
1, each stream the size of the tree, for the same-run ceiling of a kernel's byte mix,
t >= R / BW_read(s_r) + W / BW_write(s_w): dl_delta_q8_ef reads 3 streams and writes 2 (the
1 KB-per-chunk payload counted as a stream), dl_delta_q8 reads 2 and writes 1.

Method, as tools/q8_adamw_bench.py: the variants alternate, their order rotated by one every
round; two untimed rounds, then --rounds timed ones; a 1 GiB copy through other memory before
every timed launch; device events on the launch stream; medians and each variant's own
max - min. Every step runs in a fresh child process under its own time limit, and a step that
fails ends the run. No rate is claimed in advance: the result reports each encoder's fraction
of its own ceiling and whether the new one's is lower by more than dl_delta_q8's own spread.

    python tools/q8_ef_bench.py [--tree t125] [--rounds 9] [--out profiles/q8_ef_t125.json]
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
STEP_TIMEOUT_S = 240
STEPS = ("kernels", "probes")


def _stats(ms, nbytes):
    med = statistics.median(ms)
    return {"ms": [round(x, 5) for x in ms], "median_ms": round(med, 5),
            "max_minus_min_ms": round(max(ms) - min(ms), 5), "bytes": nbytes,
            "gbps_median": round(nbytes / (med * 1e-3) / 1e9, 1)}


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
    from diloco_amd.kernels import Q8_SLOT, HipKernels
    from diloco_amd.plan import SLOT_INNER, PackedTree
    from diloco_amd.trees import get_tree

    dev = torch.device("cuda", 0)
    k = HipKernels()
    numels = get_tree(args.tree).numels()
    tree = PackedTree(numels)
    elems, all_ = sum(numels), _lib.ALL_BUCKETS
    gen = torch.Generator(device=dev).manual_seed(1)
    z = dict(dtype=torch.float32, device=dev)
    theta = torch.randn(tree.total, generator=gen, **z)
    delta = torch.randn(tree.total, generator=gen, **z) * 1e-2
    offs = [int(o) for o in tree.seg_off[:-1]]
    # the inner params: one allocation per tensor, as a model's are
    inner = [(theta[o:o + n] - delta[o:o + n]).clone() for o, n in zip(offs, numels)]
    tree.bind(SLOT_INNER, inner, torch.cuda.current_stream().cuda_stream)
    wire = torch.zeros(tree.total, **z)
    resid = torch.zeros(tree.total, **z)
    slots = torch.zeros(tree.n_chunks * Q8_SLOT, dtype=torch.uint8, device=dev)
    # the reduce of one of two peers: m = half the tree's slots from each of two ranks
    m = -(-tree.n_chunks // 2)
    k.delta_q8(tree, all_, SLOT_INNER, theta, slots)
    recv = torch.cat([slots[:m * Q8_SLOT], slots[:m * Q8_SLOT]]).contiguous()
    red = torch.zeros(m * Q8_SLOT, dtype=torch.uint8, device=dev)
    resid2 = torch.zeros(m * _lib.CHUNK_ELEMS, **z)
    q8 = tree.n_chunks * Q8_SLOT
    runs = {
        "dl_delta_q8_ef": (lambda: k.delta_q8_ef(tree, all_, SLOT_INNER, theta, resid, slots),
                           q8 + 16 * elems),
        "dl_delta_q8": (lambda: k.delta_q8(tree, all_, SLOT_INNER, theta, slots), q8 + 8 * elems),
        "dl_delta_pack": (lambda: k.delta_pack(tree, all_, SLOT_INNER, theta, wire), 12 * elems),
        "dl_q8_reduce_ef": (lambda: k.q8_reduce_ef(recv, 2, m, 2, resid2, red),
                            3 * m * Q8_SLOT + 8 * m * _lib.CHUNK_ELEMS),
        "dl_q8_reduce": (lambda: k.q8_reduce(recv, 2, m, 2, red), 3 * m * Q8_SLOT),
    }
    res = _measure(runs, args.rounds)
    tree.close()
    return {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
            "elements": elems, "chunks": tree.n_chunks, "reduce_slots": m, "kernels": res}


def step_probes(args):
    import torch

    from diloco_amd import _lib
    from diloco_amd.trees import get_tree

    elems = sum(get_tree(args.tree).numels())
    stream = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(3 * elems + 64, dtype=torch.float32, device="cuda:0")

    def probe(kind, s):
        nbytes = 4 * s * elems // (16 * s) * (16 * s)  # s equal streams of whole float4s
        flags = _lib.TUNE_NT_LOADS | kind | _lib.COPY_STREAMS(s)
        src, dst = ((buf.data_ptr(), None) if kind == _lib.COPY_READ else (None, buf.data_ptr()))
        return (lambda: _lib.call("dl_copy", src, dst, nbytes, flags, stream), nbytes)

    runs = {"read_probe_3": probe(_lib.COPY_READ, 3), "read_probe_2": probe(_lib.COPY_READ, 2),
            "write_probe_2": probe(_lib.COPY_WRITE, 2), "write_probe_1": probe(_lib.COPY_WRITE, 1)}
    return {"probes": _measure(runs, args.rounds)}


def _ceiling(res, elems, q8, read_bytes, read_probe, write_probe, extra_write):
    """t >= R / BW_read + W / BW_write, in ms, from the same run's probes."""
    bw_r = res["probes"][read_probe]["gbps_median"] * 1e9
    bw_w = res["probes"][write_probe]["gbps_median"] * 1e9
    return (read_bytes * elems / bw_r + (q8 + extra_write * elems) / bw_w) * 1e3


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
            raise SystemExit("q8_ef_bench measures on the GPU; no HIP device")
        res = {"kernels": step_kernels, "probes": step_probes}[args.step](args)
        with open(args.step_out, "w") as f:
            json.dump(res, f)
        return
    res, tmp = {}, tempfile.mkdtemp(prefix="dl_q8_ef_bench_")
    for step in STEPS:  # fresh processes, each under its own limit; a failure ends the run
        part = os.path.join(tmp, step + ".json")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", args.tree,
                        "--rounds", str(args.rounds), "--step", step, "--step-out", part],
                       check=True, timeout=STEP_TIMEOUT_S)
        with open(part) as f:
            res.update(json.load(f))
    kn, elems = res["kernels"], res["elements"]
    q8 = kn["dl_delta_q8"]["bytes"] - 8 * elems
    ceil_ef = _ceiling(res, elems, q8, 12, "read_probe_3", "write_probe_2", 4)
    ceil_q8 = _ceiling(res, elems, q8, 8, "read_probe_2", "write_probe_1", 0)
    frac_ef = ceil_ef / kn["dl_delta_q8_ef"]["median_ms"]
    frac_q8 = ceil_q8 / kn["dl_delta_q8"]["median_ms"]
    # dl_delta_q8's own spread, as a fraction of its ceiling fraction
    spread = frac_q8 * kn["dl_delta_q8"]["max_minus_min_ms"] / kn["dl_delta_q8"]["median_ms"]
    out = {"tool": "tools/q8_ef_bench.py", "tree": args.tree, "rounds": args.rounds,
           "cold": "a 1 GiB copy through other memory before every timed launch",
           "not_measured": ["a multi-GPU run", "any rate of the outer step at N > 1"], **res,
           "ceiling": {
               "formula": "t >= R / BW_read(s_r) + W / BW_write(s_w), same-run dl_copy probes",
               "dl_delta_q8_ef": {"read_streams": 3, "write_streams": 2,
                                  "ceiling_ms": round(ceil_ef, 5),
                                  "fraction_of_ceiling": round(frac_ef, 4)},
               "dl_delta_q8": {"read_streams": 2, "write_streams": 1,
                               "ceiling_ms": round(ceil_q8, 5),
                               "fraction_of_ceiling": round(frac_q8, 4),
                               "own_spread_as_fraction": round(spread, 4)},
               "ef_fraction_lower_by_more_than_q8_spread": bool(frac_q8 - frac_ef > spread)},
           "reduce_ef_over_reduce_ms": round(kn["dl_q8_reduce_ef"]["median_ms"]
                                             / kn["dl_q8_reduce"]["median_ms"], 4)}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
