"""The fp4 (MXFP4) wire of the per-step DP gradient sync, without a GPU.

1. The C-ABI declares dl_gather_fp4 and dl_unpack_avg_fp4, the Python binding types them, the
   library exports them, and the ABI version is still 8; their argument checks fire before any
   device is touched.
2. The knobs: dp_wire() for fp4 with and without DILOCO_DP_FP4_EF, DP_Q8_EF ignored for fp4;
   error feedback needs a slot wire, fp4 refuses exchange="a2a"; the default wire calls no fp4
   kernel.
3. The stand-in encoder (tests/gradsync_fp4_oracle_kernels.py) equals delta_fp4 with outer = g,
   inner = +0 byte for byte, and both stand-ins stay inside the write footprint.
4. Two gloo CPU ranks through GradSync(wire_dtype="fp4") and DPSync on the checker backend, error
   feedback off and on, three consecutive syncs: .grad, both residual arenas and the averaged
   slots equal fp4_restatement.Fp4Exchange composed by hand, bit for bit; sync(max_norm) against
   the clip restatement; the error-feedback state round-trips.
5. The documented bound on |grad - mean| at n = 2 and 4, in float64, the scales read from the
   slots."""
import os
import re
import socket
import sys
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import clip_restatement as cr
import fp4_restatement as fp4
from clip_oracle_kernels import as_params
from conftest import PKG, REPO
from diloco_amd import _lib, comm, kernels
from diloco_amd.gradsync import SLOT_WIRES, GradSync
from diloco_amd.plan import SLOT_GRAD, SLOT_INNER
from gradsync_fp4_inputs import CAP, NUMELS, groupwise, special
from gradsync_fp4_oracle_kernels import NEW_METHODS, GradSyncFp4OracleKernels

F = np.float32
STEPS = 3
ALL = _lib.ALL_BUCKETS
NEW = (("dl_gather_fp4", 6), ("dl_unpack_avg_fp4", 6))


# ---- 1: the C-ABI ----------------------------------------------------------------------------
def test_abi_declares_the_gradient_entry_points():
    with open(os.path.join(REPO, "include", "diloco_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+DL_ABI_VERSION\s+8\b", header)
    assert _lib.ABI_VERSION == 8
    lib = _lib.load()
    assert lib.dl_abi_version() == 8
    for name, nargs in NEW:
        assert re.search(r"DL_API\s+int\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(lib, name), name
    for name in NEW_METHODS:
        assert callable(getattr(kernels.HipKernels, name))


def test_argument_checks_come_before_the_device():
    """No tree exists without a device, so a null tree stands in for it: the buffer checks need
    none and come first; with good buffers the null tree is reported."""
    good = [("dl_gather_fp4", (None, 0, 1, None, 64, None)),
            ("dl_gather_fp4", (None, 0, 1, 128, 64, None)),
            ("dl_unpack_avg_fp4", (None, 0, 64, 1, None, None)),
            ("dl_unpack_avg_fp4", (None, 0, 64, 1, 136, None))]
    for name, args in good:
        with pytest.raises(_lib.DilocoHipError, match="null tree") as e:
            _lib.call(name, *args)
        assert e.value.code == -1 and name in str(e.value)  # DL_E_ARG
    bad = [("dl_gather_fp4", (None, 0, 1, None, None, None), "slots is null"),
           ("dl_gather_fp4", (None, 0, 1, None, 68, None), "slots not 16-B aligned"),
           ("dl_gather_fp4", (None, 0, 1, 132, 64, None), "residual not 16-B aligned"),
           ("dl_gather_fp4", (None, 0, 1, 128, 72, None), "slots not 16-B aligned"),
           ("dl_unpack_avg_fp4", (None, 0, None, 1, None, None), "slots is null"),
           ("dl_unpack_avg_fp4", (None, 0, 68, 1, None, None), "slots not 16-B aligned"),
           ("dl_unpack_avg_fp4", (None, 0, 64, 1, 132, None), "partials not 8-B aligned")]
    for name, args, msg in bad:
        with pytest.raises(_lib.DilocoHipError, match=msg) as e:
            _lib.call(name, *args)
        assert e.value.code == (-1 if "null" in msg else -3), (name, msg)  # DL_E_ARG / DL_E_ALIGN
        assert name in str(e.value)


# ---- 2: the knobs ----------------------------------------------------------------------------
def test_dp_wire_knob(monkeypatch):
    assert comm.DP_WIRES["fp4"] == "fp4"
    monkeypatch.setattr(comm, "DP_WIRE", "fp4")
    monkeypatch.setattr(comm, "DP_FP4_EF", False)
    monkeypatch.setattr(comm, "DP_Q8_EF", True)
    assert comm.dp_wire() == ("fp4", False)  # DP_Q8_EF is the int8 wire's
    monkeypatch.setattr(comm, "DP_FP4_EF", True)
    monkeypatch.setattr(comm, "DP_Q8_EF", False)
    assert comm.dp_wire() == ("fp4", True)
    monkeypatch.setattr(comm, "DP_WIRE", "int8")
    assert comm.dp_wire() == (torch.int8, False)  # and DP_FP4_EF the fp4 wire's
    monkeypatch.setattr(comm, "DP_WIRE", "f32")
    assert comm.dp_wire() == (torch.float32, False)


def test_fp4_error_feedback_is_off_if_unset():
    import subprocess

    env = {k: v for k, v in os.environ.items() if k not in ("DILOCO_DP_FP4_EF", "DILOCO_DP_WIRE")}
    env["PYTHONPATH"] = os.pathsep.join([PKG, REPO])
    code = ("from diloco_amd import comm; print(comm.DP_WIRE, comm.DP_FP4_EF, comm.dp_wire()[0])")
    out = subprocess.run([sys.executable, "-c", code], env=env, check=True, capture_output=True,
                         text=True, timeout=120).stdout.split()
    assert out[:2] == ["f32", "False"] and out[2] == "torch.float32"
    env.update(DILOCO_DP_WIRE="fp4", DILOCO_DP_FP4_EF="1", DILOCO_DP_Q8_EF="0")
    code = "from diloco_amd import comm; print(*comm.dp_wire())"
    out = subprocess.run([sys.executable, "-c", code], env=env, check=True, capture_output=True,
                         text=True, timeout=120).stdout.split()
    assert out == ["fp4", "True"]


@pytest.mark.parametrize("wire", [torch.float32, torch.bfloat16])
def test_error_feedback_needs_a_slot_wire(wire):
    with pytest.raises(ValueError, match="fp4"):
        GradSync(as_params(groupwise(1)), None, 1, wire_dtype=wire, error_feedback=True,
                 kernels=GradSyncFp4OracleKernels())


def test_fp4_wire_refuses_the_a2a_exchange_and_other_strings():
    with pytest.raises(ValueError, match="a2a"):
        GradSync(as_params(groupwise(1)), None, 1, wire_dtype="fp4", exchange="a2a",
                 kernels=GradSyncFp4OracleKernels())
    with pytest.raises(ValueError, match="fp8"):
        GradSync(as_params(groupwise(1)), None, 1, wire_dtype="fp8",
                 kernels=GradSyncFp4OracleKernels())


def test_default_wire_calls_no_fp4_kernel():
    k = GradSyncFp4OracleKernels()
    ps = as_params(groupwise(2))
    gs = GradSync(ps, None, 1, bucket_cap_elems=CAP, kernels=k)
    assert not gs.fp4 and not gs.q8 and gs.q8_ef_state() is None
    gs.sync()
    gs.sync(1.0)
    names = [c[0] for c in k.calls]
    assert not [n for n in names if "fp4" in n or "q8" in n]
    assert "unpack_avg" in names and "unpack_avg_sumsq" in names


def test_one_replica_runs_encode_reduce_in_place_decode():
    for feedback in (False, True):
        k = GradSyncFp4OracleKernels()
        g = groupwise(3)
        ps = as_params(g)
        gs = GradSync(ps, None, 1, wire_dtype="fp4", bucket_cap_elems=CAP, kernels=k,
                      error_feedback=feedback)
        assert gs.fp4 and not gs.q8 and gs.local
        assert gs.slot_bytes == SLOT_WIRES["fp4"] == fp4.SLOT == _lib.FP4_SLOT_BYTES
        gs.sync()
        nb = gs.tree.n_buckets
        assert nb >= 2
        want = []
        for b in range(nb):
            want += [("gather_fp4", b, feedback), ("fp4_reduce", gs.q8_plan[b][1], False),
                     ("unpack_avg_fp4", b, False)]
        assert k.calls == want
        counts = [c1 - c0 for c0, c1 in gs.tree.bucket_chunks]
        ref = fp4.Fp4Exchange(NUMELS, counts, 1, ef=feedback).average([g])
        for p, w in zip(ps, ref):
            assert p.grad.numpy().tobytes() == w.tobytes()
        st = gs.q8_ef_state()
        assert (st is None) == (not feedback)
        if feedback:
            assert st["reduce"] == [] and bool(st["encode"].any())


# ---- 3: the stand-ins ------------------------------------------------------------------------
@pytest.mark.parametrize("feedback", [False, True], ids=["plain", "ef"])
def test_stand_in_encoder_equals_delta_fp4_with_a_zero_inner(feedback):
    k = GradSyncFp4OracleKernels()
    tree = k.tree(NUMELS, None, CAP)
    g = special(5)
    assert np.signbit(g[NUMELS.index(4096)][15]) and np.isnan(g[NUMELS.index(4096)]).any()
    grads = [torch.from_numpy(x.copy()) for x in g]
    k.bind(tree, SLOT_GRAD, grads, None)
    k.bind(tree, SLOT_INNER, [torch.zeros(n) for n in NUMELS], None)
    theta = torch.zeros(tree.total)
    r0 = torch.zeros(tree.total)
    for o, x, r in zip(tree.seg_off[:-1], g, groupwise(6, lo=-5.0, hi=-4.0)):
        theta[int(o):int(o) + x.size] = torch.from_numpy(x)
        r0[int(o):int(o) + x.size] = torch.from_numpy(r)
    a = torch.full((tree.n_chunks * fp4.SLOT,), 0xEE, dtype=torch.uint8)
    b = a.clone()
    ra, rb = (r0.clone(), r0.clone()) if feedback else (None, None)
    k.gather_fp4(tree, ALL, SLOT_GRAD, ra, a)
    k.delta_fp4(tree, ALL, SLOT_INNER, theta, rb, b)
    assert a.numpy().tobytes() == b.numpy().tobytes() and not (a == 0xEE).all()
    if feedback:
        assert fp4.same_bits(ra.numpy(), rb.numpy()) and not torch.equal(ra, r0)
    # the gradients are only read
    assert all(fp4.same_bits(t.numpy(), x) for t, x in zip(grads, g))


@pytest.mark.parametrize("row", ["gather_fp4", "gather_fp4_ef", "unpack_avg_fp4",
                                 "unpack_avg_fp4_sumsq"])
def test_reference_stays_inside_its_footprint(row):
    """The CPU stand-ins that tests/test_gradsync_fp4_gpu.py compares the kernels' footprints
    with write nothing outside the documented outputs themselves (both sentinels, the mixed
    placement)."""
    import gradsync_fp4_footprint as gf

    for case in gf.ROWS[row]():
        gf.run_case(case, places=case.places[2:])


# ---- 4: gloo CPU ranks -----------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _flat(ps):
    return np.concatenate([p.grad.detach().numpy().reshape(-1) for p in ps])


def _worker(rank, world, port, feedback, out):
    for p in (PKG, REPO, os.path.join(REPO, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    torch.set_num_threads(1)
    for v in ("DILOCO_DP_EXCHANGE", "DILOCO_DP_WIRE", "DILOCO_DP_Q8_EF", "DILOCO_DP_FP4_EF"):
        os.environ.pop(v, None)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank,
                            world_size=world)
    k = GradSyncFp4OracleKernels()
    kernels.set_default_kernels(k)
    rec = {}
    params = [torch.nn.Parameter(torch.zeros(n)) for n in NUMELS]
    gs = GradSync(params, None, world, wire_dtype="fp4", bucket_cap_elems=CAP,
                  error_feedback=feedback)
    counts = [c1 - c0 for c0, c1 in gs.tree.bucket_chunks]
    rec["counts"] = np.array(counts)
    ex = fp4.Fp4Exchange(NUMELS, counts, world, ef=feedback)
    rec["state_is_none"] = np.array(gs.q8_ef_state() is None)

    def step(s, clip_factor=None):
        by_rank = [groupwise(1000 * s + r) for r in range(world)]
        for p, g in zip(params, by_rank[rank]):
            p.grad = torch.from_numpy(g.copy())  # a fresh tensor every step
        want = ex.average(by_rank)
        if clip_factor is None:
            assert gs.sync() is None
        else:
            norm0, _ = cr.norm_and_coef(want, 1.0)
            max_norm = float(norm0) * clip_factor
            norm, coef, want = cr.clip(want, max_norm)
            got = gs.sync(max_norm)
            rec[f"norm_s{s}"] = np.array([np.float32(got.item()), norm])
            rec[f"clipped_s{s}"] = np.array(bool(coef < 1))
        rec[f"grad_s{s}"] = _flat(params)
        rec[f"ref_s{s}"] = np.concatenate(want)
        # the averaged slots this rank holds (padding slots left out), and the restatement's
        rec[f"slots_s{s}"] = np.concatenate(
            [gs.q8_region(b)[:c * fp4.SLOT].numpy() for b, c in enumerate(counts)])
        rec[f"ref_slots_s{s}"] = np.concatenate(ex.avg_slots)

    step(1)
    step(2, 0.5)  # clips
    step(3, 2.0)  # does not
    rec["calls"] = np.array([c[0] for c in k.calls])
    rec["ef_flags"] = np.array([bool(c[2]) for c in k.calls if c[0] in ("gather_fp4", "fp4_reduce")])
    rec["partials_flags"] = np.array([bool(c[2]) for c in k.calls if c[0] == "unpack_avg_fp4"])
    if feedback:
        st = gs.q8_ef_state()
        rec["encode"] = st["encode"].numpy()
        rec["ref_encode"] = np.zeros(gs.tree.total, dtype=F)
        for t, o in enumerate(gs.tree.seg_off[:-1]):
            rec["ref_encode"][int(o):int(o) + NUMELS[t]] = ex.enc[rank][t]
        rec["reduce"] = np.concatenate([a.numpy() for a in st["reduce"]])
        rec["ref_reduce"] = np.concatenate([ex.red[b][rank] for b in range(len(counts))])
        gs.load_q8_ef_state(None)
        z = gs.q8_ef_state()
        rec["reset"] = np.array(not z["encode"].any() and not any(a.any() for a in z["reduce"]))
        gs.load_q8_ef_state(st)
        back = gs.q8_ef_state()
        rec["round_trip"] = np.array(
            back["encode"].numpy().tobytes() == rec["encode"].tobytes()
            and all(a.numpy().tobytes() == b.numpy().tobytes()
                    for a, b in zip(back["reduce"], st["reduce"])))
        raised = []
        for bad in (dict(st, encode=st["encode"][:-1]), dict(st, reduce=st["reduce"][:-1]),
                    dict(st, reduce=[a[:-1] for a in st["reduce"]])):
            try:
                gs.load_q8_ef_state(bad)
                raised.append(False)
            except ValueError:
                raised.append(True)
        rec["mismatch_raises"] = np.array(all(raised))
        step(4)  # continues as if the state had never left
    # DPSync under DP_WIRE=fp4 builds this exchange (zero residuals: a fresh restatement); under
    # the default wire it calls no fp4 kernel
    model = torch.nn.Module()
    model.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(n)) for n in NUMELS])
    w = SimpleNamespace(stage2ranks={0: list(range(world))}, stage=0, curr_stage_group=None)
    comm.DP_WIRE, comm.DP_FP4_EF, comm.DP_Q8_EF = "fp4", feedback, not feedback
    dp = comm.DPSync(w)
    by_rank = [groupwise(77 + r) for r in range(world)]
    for p, g in zip(model.parameters(), by_rank[rank]):
        p.grad = torch.from_numpy(g.copy())
    del k.calls[:]
    assert dp.sync_gradients(model) is None
    dgs = next(iter(dp._grad_syncs.values()))
    dcounts = [c1 - c0 for c0, c1 in dgs.tree.bucket_chunks]
    rec["dp_fp4"] = np.array(dgs.fp4 and not dgs.q8 and dgs.error_feedback == feedback)
    rec["dp_grad"] = _flat(list(model.parameters()))
    rec["dp_ref"] = np.concatenate(
        fp4.Fp4Exchange(NUMELS, dcounts, world, ef=feedback).average(by_rank))
    rec["dp_calls"] = np.array([c[0] for c in k.calls])
    comm.DP_WIRE = "f32"
    del k.calls[:]
    comm.DPSync(w).sync_gradients(model)
    rec["dp_default_calls"] = np.array([c[0] for c in k.calls])
    np.savez(os.path.join(out, f"r{rank}.npz"), **rec)
    dist.barrier()
    dist.destroy_process_group()


_RUNS = {}


def _run(world, feedback):
    """One run per (world, feedback), shared by the tests that read it."""
    key = (world, feedback)
    if key not in _RUNS:
        out = tempfile.mkdtemp(prefix="dl_gradsync_fp4_")
        # forked workers, as tests/test_dist_gloo.py: CPU only, no HIP state to inherit
        mp.start_processes(_worker, args=(world, _free_port(), feedback, out), nprocs=world,
                           join=True, start_method="fork")
        _RUNS[key] = [dict(np.load(os.path.join(out, f"r{r}.npz"))) for r in range(world)]
    return _RUNS[key]


@pytest.mark.parametrize("feedback", [False, True], ids=["plain", "ef"])
def test_gloo_ranks_match_the_exchange_composed_by_hand(feedback):
    recs = _run(2, feedback)
    counts = [int(c) for c in recs[0]["counts"]]
    assert len(counts) >= 2 and any(c % 2 for c in counts), counts
    for rec in recs:
        assert bool(rec["state_is_none"]) == (not feedback)
        for s in range(1, STEPS + 1 + int(feedback)):
            got, want = rec[f"grad_s{s}"], rec[f"ref_s{s}"]
            assert got.tobytes() == want.tobytes(), (s, int((got != want).sum()))
            assert got.tobytes() == recs[0][f"grad_s{s}"].tobytes(), s
            # byte-identical averaged slots on both ranks, the restatement's
            assert rec[f"slots_s{s}"].tobytes() == rec[f"ref_slots_s{s}"].tobytes(), s
            assert rec[f"slots_s{s}"].tobytes() == recs[0][f"slots_s{s}"].tobytes(), s
            assert rec[f"grad_s{s}"].any()
        # sync(max_norm) is sync() then the clip restatement: the norm too
        assert bool(rec["clipped_s2"]) and not bool(rec["clipped_s3"])
        for s in (2, 3):
            got, want = rec[f"norm_s{s}"]
            assert got.tobytes() == want.tobytes(), s
        calls = [str(c) for c in rec["calls"]]
        nb = len(counts)
        for name in ("gather_fp4", "fp4_reduce", "unpack_avg_fp4"):
            assert calls.count(name) == nb * STEPS, name
        assert (rec["ef_flags"] == feedback).all()
        assert rec["partials_flags"].tolist() == [False] * nb + [True] * (2 * nb)
        assert calls.count("norm_finish") == 2 and calls.count("scale_by") == 2
        assert not [c for c in calls if "q8" in c or c in ("grad_sumsq", "unpack_avg", "gather")]


def test_error_feedback_state_round_trips():
    for rec in _run(2, True):
        assert rec["encode"].tobytes() == rec["ref_encode"].tobytes() and rec["encode"].any()
        assert rec["reduce"].tobytes() == rec["ref_reduce"].tobytes() and rec["reduce"].any()
        assert bool(rec["reset"]) and bool(rec["round_trip"]) and bool(rec["mismatch_raises"])


@pytest.mark.parametrize("feedback", [False, True], ids=["plain", "ef"])
def test_dpsync_takes_the_wire_from_its_knobs(feedback):
    recs = _run(2, feedback)
    for rec in recs:
        assert bool(rec["dp_fp4"])
        assert rec["dp_grad"].tobytes() == rec["dp_ref"].tobytes()
        assert rec["dp_grad"].tobytes() == recs[0]["dp_grad"].tobytes()
        calls = [str(c) for c in rec["dp_calls"]]
        assert "gather_fp4" in calls and "fp4_reduce" in calls and "unpack_avg_fp4" in calls
        assert "gather" not in calls and not [c for c in calls if "q8" in c]
        default = [str(c) for c in rec["dp_default_calls"]]
        assert default and not [c for c in default if "fp4" in c or "q8" in c]


# ---- 5: the documented bound -----------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("length", [1, 33, 4095, 4096])
def test_documented_error_bound(n, length):
    """|grad_i - mean_r x_r,i| <= (1/n) Σ_r 2^(E_r(G)-127) + 2^(E_red(G)-127)
                                   + n · 2^-24 · max_r |deq_r,i|
    Each peer's decoded value is within its group's scale of x_r (the codec's bound: the nearest
    grid point of a grid whose neighbours are at most 2 scales apart); the mean of the decoded
    values is then within the mean of the scales; the fp32 rank-order sum makes n - 1 roundings
    of partial sums of magnitude at most n·max|deq| and the division one more of a value at most
    max|deq|: after the division at most n · 2^-24 · max|deq| together; the re-quantiser of the
    average adds at most its own scale. The scales are read from the slots, everything in
    float64; magnitudes stay in the normal range, where an fp32 rounding is relative."""
    by_rank = [groupwise(10 * n + r + length, [length], lo=-6.0 + r, hi=2.0 + r)[0]
               for r in range(n)]
    slots = [fp4.encode_values(x) for x in by_rank]
    red, _ = fp4.reduce_slots(np.concatenate(slots), n, 1, n)
    grad = fp4.decode_slot(red, length).astype(np.float64)
    mean = np.mean(np.stack(by_rank).astype(np.float64), axis=0)

    def scales(slot):
        return np.ldexp(1.0, np.repeat(slot[:fp4.N_GROUPS].astype(np.int64), 32) - 127)[:length]

    e_peers = np.stack([s[:-(-length // 32)] for s in slots])
    if length > 32:  # some group carries a different E on different peers
        assert (e_peers.max(axis=0) != e_peers.min(axis=0)).any()
    deq_max = np.max(np.abs(np.stack([fp4.decode_slot(s, length) for s in slots])), axis=0)
    bound = (sum(scales(s) for s in slots) / n + scales(red)
             + n * 2.0 ** -24 * deq_max.astype(np.float64))
    err = np.abs(grad - mean)
    print(f"n {n} len {length}: max error / bound {float((err / bound).max()):.4f}")
    assert (err <= bound).all()
