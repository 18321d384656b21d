#!/usr/bin/env python3
"""Rates of the two flat-shard AdamW kernels on ONE GPU, launched directly on synthetic data.

dl_shard_adamw and dl_shard_reduce_adamw at the T125 whole-tree size and at 1/8 of it (a
rank's shard at eight peers), beside dl_unpack_adamw over the T125 tree with inner_slot -1 (the
same 28 B/param mix under the tree walker) and dl_copy with its read and write probes at the
same sizes, all in one process. The kernels alternate (the order reversed every other round);
each timed launch is one kernel between two device events, after a synchronise and after a
1 GiB copy through other memory, so every launch starts with the Infinity Cache holding none
of its operands (the 1/8-size working set would otherwise fit in it). Two untimed rounds load
the code objects. Every sample is kept; rates are over the median, over the bytes the
algorithm needs:

    dl_shard_adamw / dl_unpack_adamw   28 B per element (fp32 wire: 16 read, 12 written)
    dl_shard_reduce_adamw              4 n + 12 read, 12 + 4 (avg_out) written
    dl_copy                            4 read, 4 written

`vs_copy` is a kernel's rate over the same run's fastest dl_copy rate at that size;
`vs_mix_ceiling` is the least time R / BW_read + W / BW_write (the probes' rates at that size)
over the kernel's time. `spread` is (max - min) / median of a kernel's own samples.

Not measured here, and nowhere else so far: a multi-GPU run, and any rate of the outer step at
N > 1 (the collectives, the all_gather of θ, the overlap between buckets).

    python tools/shard_adamw_rate.py [--rounds 9] [--tree t125] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "diloco-swarm_amd"))

import torch  # noqa: E402

from diloco_amd import _lib  # noqa: E402
from diloco_amd.kernels import HipKernels, adamw_scalars  # noqa: E402
from diloco_amd.plan import PackedTree  # noqa: E402
from diloco_amd.trees import get_tree  # noqa: E402

HBM_PEAK = 8e12  # B/s
SLICES = (2, 8)
FLUSH_BYTES = 1 << 30


def _stats(ms, nbytes):
    med = statistics.median(ms)
    return {"ms": [round(x, 5) for x in ms], "median_ms": round(med, 5),
            "spread": round((max(ms) - min(ms)) / med, 4), "bytes": nbytes,
            "gbps_median": round(nbytes / (med * 1e-3) / 1e9, 1),
            "fraction_of_8TBps": round(nbytes / (med * 1e-3) / HBM_PEAK, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--tree", default="t125")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shard_adamw_rate measures on the GPU; no HIP device")
    dev = torch.device("cuda", 0)
    k = HipKernels()
    spec = get_tree(args.tree)
    tree = PackedTree(spec.numels())
    elems = sum(spec.numels())
    whole = elems // 64 * 64  # the flat sizes: whole tree, and a rank's shard at eight peers
    sizes = {"whole": whole, "eighth": whole // 8}
    gen = torch.Generator(device=dev).manual_seed(1)
    z = dict(dtype=torch.float32, device=dev)

    def rand(n, scale=1.0):
        return torch.randn(n, generator=gen, **z) * scale

    total = max(tree.total, whole)
    theta, m1, m2, avg = rand(total), torch.zeros(total, **z), torch.zeros(total, **z), \
        torch.zeros(total, **z)
    slices = rand(max(SLICES) * whole, 1e-2)  # the first n * len elements are the n slices
    wire = slices[:total]
    dst = torch.empty(total, **z)
    flush_a = torch.zeros(FLUSH_BYTES // 4, **z)
    flush_b = torch.empty_like(flush_a)
    stream = torch.cuda.current_stream().cuda_stream
    step = [0]

    def sc():
        step[0] += 1  # AdamW's bias corrections move with the step count, as in a run
        return adamw_scalars(0.01, 0.9, 0.95, 0.1, 1e-8, float(step[0]))

    def copy(n, flags):
        return lambda: _lib.call("dl_copy", wire.data_ptr(), dst.data_ptr(), 4 * n, flags, stream)

    runs = {}  # name -> (launch, bytes)
    runs["dl_unpack_adamw@tree"] = (
        lambda: k.unpack_adamw(tree, _lib.ALL_BUCKETS, wire, 2, theta, m1, m2, sc(), -1),
        28 * elems)
    for tag, n in sizes.items():
        runs[f"dl_shard_adamw@{tag}"] = (
            lambda n=n: k.shard_adamw(wire[:n], 2, theta[:n], m1[:n], m2[:n], sc()), 28 * n)
        for ns in SLICES:
            runs[f"dl_shard_reduce_adamw_n{ns}@{tag}"] = (
                lambda n=n, ns=ns: k.shard_reduce_adamw(slices[:ns * n], ns, theta[:n], m1[:n],
                                                        m2[:n], sc(), avg_out=avg[:n]),
                (4 * ns + 12 + 16) * n)
        nt = _lib.TUNE_NT_LOADS
        runs[f"dl_copy@{tag}"] = (copy(n, nt), 8 * n)
        runs[f"dl_copy_wide@{tag}"] = (copy(n, nt | _lib.COPY_WIDE), 8 * n)
        runs[f"read_probe_4@{tag}"] = (copy(n // 64 * 64, nt | _lib.COPY_READ
                                            | _lib.COPY_STREAMS(4)), 4 * (n // 64 * 64))
        runs[f"write_probe_3@{tag}"] = (copy(n // 48 * 48, nt | _lib.COPY_WRITE
                                             | _lib.COPY_STREAMS(3)), 4 * (n // 48 * 48))
    ms = {name: [] for name in runs}
    for r in range(args.rounds + 2):
        names = list(runs)
        if r % 2:
            names.reverse()
        for name in names:
            flush_b.copy_(flush_a)  # the operands leave the Infinity Cache
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            runs[name][0]()
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:  # the first two rounds load the code objects
                ms[name].append(e0.elapsed_time(e1))
    res = {name: _stats(ms[name], runs[name][1]) for name in runs}
    for tag, n in sizes.items():
        cp = max(res[f"dl_copy@{tag}"]["gbps_median"], res[f"dl_copy_wide@{tag}"]["gbps_median"])
        bw_r = res[f"read_probe_4@{tag}"]["gbps_median"] * 1e9
        bw_w = res[f"write_probe_3@{tag}"]["gbps_median"] * 1e9
        mixes = {f"dl_shard_adamw@{tag}": (16 * n, 12 * n)}
        for ns in SLICES:
            mixes[f"dl_shard_reduce_adamw_n{ns}@{tag}"] = ((4 * ns + 12) * n, 16 * n)
        if tag == "whole":
            mixes["dl_unpack_adamw@tree"] = (16 * elems, 12 * elems)
        for name, (rd, wr) in mixes.items():
            floor_ms = (rd / bw_r + wr / bw_w) * 1e3
            res[name]["vs_copy"] = round(res[name]["gbps_median"] / cp, 4)
            res[name]["vs_mix_ceiling"] = round(floor_ms / res[name]["median_ms"], 4)
    sa, ua = res["dl_shard_adamw@whole"], res["dl_unpack_adamw@tree"]
    out = {"tool": "tools/shard_adamw_rate.py", "tree": args.tree,
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "rounds": args.rounds, "elements": {"tree": elems, **sizes},
           "cold": "a 1 GiB copy through other memory before every timed launch",
           "not_measured": ["a multi-GPU run", "any rate of the outer step at N > 1"],
           "kernels": res,
           "shard_adamw_over_unpack_adamw_rate": round(sa["gbps_median"] / ua["gbps_median"], 4),
           "unpack_adamw_own_spread": ua["spread"]}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    tree.close()


if __name__ == "__main__":
    main()
