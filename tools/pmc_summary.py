#!/usr/bin/env python3
"""Per-launch HBM bytes of the outer-step kernels from rocprofv3 --pmc passes.

    python tools/pmc_summary.py <fetch_counter_collection.csv> <write_counter_collection.csv> \
        <tree> <out.json>

gfx950 correction (MI355X_MICROARCH.md §HBM): FETCH_SIZE (KiB) reports exactly half the bytes
of a wide coalesced streaming read -> x2. WRITE_SIZE (KiB) is exact for 16-B-per-lane stores.
Counters are summed over the dimensions rocprofv3 reports per dispatch, then averaged over the
dispatches of each kernel.
"""
import csv
import re
import json
import sys
from collections import defaultdict


def short(name):
    # the outer-step body (csrc/dl_outer_step.h): OuterStep<gradient source, update rule> under
    # k_walk, or under k_flat for dl_shard_sgd; SgdRule's MODE 1 is the first step
    m = re.search(r"FromDeltaAfterPending<[^<]*SgdRule<(\d)> >,[^<]*SgdRule<\d>", name)
    if m:  # the step after a deferred one; the pending rule's MODE 1: that one was the first
        return "delta_pack_sgd_resume" + ("_after_first" if m.group(1) == "1" else "")
    m = re.search(r"OuterStep<.*?\b(FromWire|FromDeltaKeptOnWire|FromDelta)\b.*?"
                  r"\b(AdamRule|SgdRule<(\d)>)", name)
    if m:
        src = {"FromWire": "unpack", "FromDelta": "delta", "FromDeltaKeptOnWire": "delta_pack"}
        v = "shard_sgd" if "k_flat" in name else src[m.group(1)] + (
            "_adamw" if m.group(2) == "AdamRule" else "_sgd")
        if re.search(r"SgdRule<\d>, true>", name):  # kDefer: θ and the momentum not stored
            v += "_defer"
        return v + ("_first" if m.group(3) == "1" else "")
    # most specific first: UnpackSgdQ8 before the plain bodies, DeltaPackPair before DeltaPack
    names = {"k_xgmi_reduce_sgd": "xgmi_reduce_sgd", "DeltaQ8": "delta_q8", "UnpackSgdQ8": "unpack_sgd_q8",
             "k_q8_reduce": "q8_reduce",
             "DeltaPackPair": "delta_pack_pairs", "GatherPair": "gather_pairs",
             "DeltaPack": "delta_pack",
             "UnpackAvg": "unpack_avg", "Gather": "gather",
             "Scatter": "scatter", "k_fill_synth": "fill_synth",
             "k_serialize_f32x4": "serialize_f32", "k_serialize<unsigned short>": "serialize_bf16",
             "k_slices_sgd": "shard_reduce_sgd"}
    if "k_xgmi_reduce_sgd" in name and ", true>" in name:
        return "xgmi_delta_sgd"  # the pack-free variant (exchange="xgmi_inner")
    for k, v in names.items():
        if k in name:
            # these SGD kernels' MODE (1 = first step) is the last argument of their own
            # template list (k_walk's trailing arguments are the load / store policy)
            m = re.search(re.escape(k) + r"<([^<>]*)>", name)
            first = (k in ("UnpackSgdQ8", "k_slices_sgd")
                     and m is not None and m.group(1).split(",")[-1].strip() == "1")
            if k == "k_slices_sgd" and m is not None:  # the slice count is its first argument
                nsl = m.group(1).split(",")[0].strip()
                v += "" if nsl == "1" else f"_n{nsl}"
            return v + ("_first" if first else "")
    return None


def load(path, counter):
    per = defaultdict(float)  # (kernel, dispatch) -> value
    for r in csv.DictReader(open(path)):
        if r.get("Counter_Name") != counter:
            continue
        k = short(r["Kernel_Name"])
        if k is None:
            continue
        per[(k, r["Dispatch_Id"])] += float(r["Counter_Value"])
    agg = defaultdict(list)
    for (k, _d), v in per.items():
        agg[k].append(v)
    return {k: sum(v) / len(v) for k, v in agg.items()}


def main():
    fpath, wpath, tree, out = sys.argv[1:5]
    f = load(fpath, "FETCH_SIZE")
    w = load(wpath, "WRITE_SIZE")
    res = {"tree": tree, "unit": "bytes per launch", "correction": "FETCH_SIZE x2 (gfx950)",
           "kernels": {}}
    for k in sorted(set(f) | set(w)):
        fb = f.get(k, 0.0) * 1024 * 2
        wb = w.get(k, 0.0) * 1024
        res["kernels"][k] = {"fetch_bytes": fb, "write_bytes": wb, "hbm_bytes": fb + wb}
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
