"""The int8 wire of the per-step DP gradient sync, without a GPU.

1. The C-ABI declares dl_gather_q8, dl_gather_q8_ef and dl_unpack_avg_q8, the Python binding
   types them, the library exports them, and the ABI version is still 8.
2. Their argument checks fire before any device is touched.
3. The knobs: error feedback needs int8, int8 refuses exchange="a2a", an unknown DILOCO_DP_WIRE
   raises, and the default wire calls no int8 kernel.
4. The plain codec's error bound on the restatement (oracle.q8_average).
5. Gloo CPU ranks (n = 2, 3) through GradSync(wire_dtype=torch.int8) and DPSync on the checker
   backend (tests/gradsync_q8_oracle_kernels.py): .grad byte-identical on every rank and equal
   to the exchange composed by hand; sync(max_norm) against the clip restatement; the
   error-feedback state round-trips."""
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
import q8_ef_restatement as ef
from clip_oracle_kernels import as_params
from conftest import PKG, REPO
from diloco_amd import _lib, comm, kernels
from diloco_amd.gradsync import GradSync
from gradsync_q8_oracle_kernels import NEW_METHODS, GradSyncQ8OracleKernels
from oracle import oracle

F = np.float32
NUMELS = [1, 3, 257, 4095, 4096, 4097, 8197]
CAP = 4096
STEPS = 3
NEW = (("dl_gather_q8", 5), ("dl_gather_q8_ef", 6), ("dl_unpack_avg_q8", 6))


# ---- 1, 2: the C-ABI -------------------------------------------------------------------------
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
    good = {"dl_gather_q8": (None, 0, 1, 64, None),
            "dl_gather_q8_ef": (None, 0, 1, 128, 64, None),
            "dl_unpack_avg_q8": (None, 0, 64, 1, None, None)}
    for name, args in good.items():
        with pytest.raises(_lib.DilocoHipError, match="null tree") as e:
            _lib.call(name, *args)
        assert e.value.code == -1 and name in str(e.value)  # DL_E_ARG
    bad = [("dl_gather_q8", (None, 0, 1, None, None), "slots is null"),
           ("dl_gather_q8", (None, 0, 1, 68, None), "slots not 16-B aligned"),
           ("dl_gather_q8_ef", (None, 0, 1, None, 64, None), "residual is null"),
           ("dl_gather_q8_ef", (None, 0, 1, 132, 64, None), "residual not 16-B aligned"),
           ("dl_gather_q8_ef", (None, 0, 1, 128, None, None), "slots is null"),
           ("dl_gather_q8_ef", (None, 0, 1, 128, 72, None), "slots not 16-B aligned"),
           ("dl_unpack_avg_q8", (None, 0, None, 1, None, None), "slots is null"),
           ("dl_unpack_avg_q8", (None, 0, 68, 1, None, None), "slots not 16-B aligned"),
           ("dl_unpack_avg_q8", (None, 0, 64, 1, 132, None), "partials not 8-B aligned")]
    for name, args, msg in bad:
        with pytest.raises(_lib.DilocoHipError, match=msg) as e:
            _lib.call(name, *args)
        assert e.value.code == (-1 if "null" in msg else -3), (name, msg)  # DL_E_ARG / DL_E_ALIGN
        assert name in str(e.value)


# ---- 3: the knobs ----------------------------------------------------------------------------
def _grads(seed, numels=NUMELS):
    """Gradients with one element of ~1 per 1500 and ~1e-3 elsewhere: most elements quantise to
    0 and live on in the residual."""
    rng = np.random.default_rng(seed)
    out = []
    for n in numels:
        g = (1e-3 * rng.standard_normal(n)).astype(F)
        g[::1500] = 1.0 + rng.random(g[::1500].size).astype(F)
        out.append(g)
    return out


@pytest.mark.parametrize("wire", [torch.float32, torch.bfloat16])
def test_error_feedback_needs_the_int8_wire(wire):
    with pytest.raises(ValueError, match="int8"):
        GradSync(as_params(_grads(1)), None, 1, wire_dtype=wire, error_feedback=True,
                 kernels=GradSyncQ8OracleKernels())


def test_int8_wire_refuses_the_a2a_exchange():
    with pytest.raises(ValueError, match="a2a"):
        GradSync(as_params(_grads(1)), None, 1, wire_dtype=torch.int8, exchange="a2a",
                 kernels=GradSyncQ8OracleKernels())


def test_dp_wire_knob(monkeypatch):
    assert comm.DP_WIRE == os.environ.get("DILOCO_DP_WIRE", "f32")
    monkeypatch.setattr(comm, "DP_WIRE", "f32")
    monkeypatch.setattr(comm, "DP_Q8_EF", True)
    assert comm.dp_wire() == (torch.float32, False)  # consulted for int8 only
    monkeypatch.setattr(comm, "DP_WIRE", "bf16")
    assert comm.dp_wire() == (torch.bfloat16, False)
    monkeypatch.setattr(comm, "DP_WIRE", "int8")
    assert comm.dp_wire() == (torch.int8, True)
    monkeypatch.setattr(comm, "DP_Q8_EF", False)
    assert comm.dp_wire() == (torch.int8, False)
    monkeypatch.setattr(comm, "DP_WIRE", "fp8")
    with pytest.raises(ValueError, match="DILOCO_DP_WIRE"):
        comm.dp_wire()


def test_default_wire_calls_no_int8_kernel():
    k = GradSyncQ8OracleKernels()
    ps = as_params(_grads(2))
    gs = GradSync(ps, None, 1, bucket_cap_elems=CAP, kernels=k)
    assert not gs.q8 and gs.q8_ef_state() is None
    gs.sync()
    gs.sync(1.0)
    gs.load_q8_ef_state(None)
    with pytest.raises(ValueError, match="without int8 error feedback"):
        gs.load_q8_ef_state({"encode": torch.zeros(1), "reduce": []})
    names = [n for n, _ in k.calls]
    assert not [n for n in names if "q8" in n]
    assert "unpack_avg" in names and "unpack_avg_sumsq" in names


# ---- 4: the plain codec's error bound --------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("length", [1, 5, 257, 4095, 4096])
def test_plain_codec_error_bound(n, length):
    """|avg_int8 - mean_r g_r| <= (A/127)(1 + 1/254) + slack per element, A = max_r amax_r.

    Two half-steps: every rank's quantiser is off by at most s_r/2 <= A/254, and so is the mean
    of the dequantised values; the re-quantiser of the average adds half a step of its own
    amax, which is at most A(1 + 1/254). The fp32 slack counts the roundings of values of
    magnitude at most B = A(1 + 1/254), each at most 2^-24 of its value: per rank the scale,
    x / s (127 s 2^-24 <= B 2^-24 once multiplied by s) and float(q)·s: 3; the rank-order sum:
    n - 1 additions of partial sums up to n B: n(n - 1); the division by n: 1; the second
    quantiser's scale, division and product: 3. K = 7 + n(n - 1), slack = K · 2^-24 · B."""
    rng = np.random.default_rng(100 * n + length)
    grads = []
    for r in range(n):
        g = ((0.5 + r) * rng.standard_normal(length)).astype(F)
        g[rng.integers(length)] = (3.0 + r) * (-1) ** r
        grads.append(g)
    avg = oracle.q8_average([[g] for g in grads], [length], [1])[0]
    mean = np.mean(np.stack(grads).astype(np.float64), axis=0)
    a = max(float(np.abs(g).max()) for g in grads)
    b = a * (1 + 1 / 254)
    slack = (7 + n * (n - 1)) * 2.0 ** -24 * b
    err = float(np.abs(avg.astype(np.float64) - mean).max())
    print(f"n {n} len {length}: error {err:.6g}, bound {a / 127 * (1 + 1 / 254) + slack:.6g}")
    assert err <= a / 127 * (1 + 1 / 254) + slack


# ---- 5: gloo CPU ranks -----------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _flat(ps):
    return np.concatenate([p.grad.detach().numpy().reshape(-1) for p in ps])


class _Reference:
    """The exchange composed by hand: EFExchange with error feedback, oracle.q8_average
    without."""

    def __init__(self, counts, world, feedback):
        self.counts, self.feedback = counts, feedback
        self.ex = ef.EFExchange(NUMELS, counts, world) if feedback else None

    def average(self, by_rank):
        if self.feedback:
            return self.ex.average(by_rank)
        return oracle.q8_average(by_rank, NUMELS, self.counts)


def _worker(rank, world, port, feedback, out):
    for p in (PKG, REPO, os.path.join(REPO, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    torch.set_num_threads(1)
    for v in ("DILOCO_DP_EXCHANGE", "DILOCO_DP_WIRE", "DILOCO_DP_Q8_EF"):
        os.environ.pop(v, None)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank,
                            world_size=world)
    k = GradSyncQ8OracleKernels()
    kernels.set_default_kernels(k)
    rec = {}
    params = [torch.nn.Parameter(torch.zeros(n)) for n in NUMELS]
    gs = GradSync(params, None, world, wire_dtype=torch.int8, bucket_cap_elems=CAP,
                  error_feedback=feedback)
    counts = [c1 - c0 for c0, c1 in gs.tree.bucket_chunks]
    rec["counts"] = np.array(counts)
    ref = _Reference(counts, world, feedback)
    rec["state_is_none"] = np.array(gs.q8_ef_state() is None)

    def step(s, clip_factor=None):
        by_rank = [_grads(1000 * s + r) for r in range(world)]
        for p, g in zip(params, by_rank[rank]):
            p.grad = torch.from_numpy(g.copy())  # a fresh tensor every step
        want = ref.average(by_rank)
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

    step(1)
    step(2, 0.5)  # clips
    step(3, 2.0)  # does not
    rec["calls"] = np.array([c[0] for c in k.calls])
    if feedback:
        st = gs.q8_ef_state()
        rec["encode"] = st["encode"].numpy()
        rec["ref_encode"] = np.zeros(gs.tree.total, dtype=F)
        for t, o in enumerate(gs.tree.seg_off[:-1]):
            rec["ref_encode"][int(o):int(o) + NUMELS[t]] = ref.ex.enc[rank][t]
        rec["reduce"] = np.concatenate([a.numpy() for a in st["reduce"]])
        rec["ref_reduce"] = np.concatenate([ref.ex.red[b][rank] for b in range(len(counts))])
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
    # DPSync under DP_WIRE=int8 builds this exchange (zero residuals: a fresh reference); under
    # the default wire it calls no int8 kernel
    model = torch.nn.Module()
    model.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(n)) for n in NUMELS])
    w = SimpleNamespace(stage2ranks={0: list(range(world))}, stage=0, curr_stage_group=None)
    comm.DP_WIRE, comm.DP_Q8_EF = "int8", feedback
    dp = comm.DPSync(w)
    by_rank = [_grads(77 + r) for r in range(world)]
    for p, g in zip(model.parameters(), by_rank[rank]):
        p.grad = torch.from_numpy(g.copy())
    del k.calls[:]
    assert dp.sync_gradients(model) is None
    dgs = next(iter(dp._grad_syncs.values()))
    dcounts = [c1 - c0 for c0, c1 in dgs.tree.bucket_chunks]
    rec["dp_q8"] = np.array(dgs.q8 and dgs.error_feedback == feedback)
    rec["dp_grad"] = _flat(list(model.parameters()))
    rec["dp_ref"] = np.concatenate(_Reference(dcounts, world, feedback).average(by_rank))
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
        out = tempfile.mkdtemp(prefix="dl_gradsync_q8_")
        # forked workers, as tests/test_dist_gloo.py: CPU only, no HIP state to inherit
        mp.start_processes(_worker, args=(world, _free_port(), feedback, out), nprocs=world,
                           join=True, start_method="fork")
        _RUNS[key] = [dict(np.load(os.path.join(out, f"r{r}.npz"))) for r in range(world)]
    return _RUNS[key]


@pytest.mark.parametrize("feedback", [False, True])
@pytest.mark.parametrize("world", [2, 3])
def test_gloo_ranks_match_the_exchange_composed_by_hand(world, feedback):
    recs = _run(world, feedback)
    counts = [int(c) for c in recs[0]["counts"]]
    assert len(counts) >= 2 and any(c % world for c in counts), counts
    for rec in recs:
        assert bool(rec["state_is_none"]) == (not feedback)
        for s in range(1, STEPS + 1 + int(feedback)):
            got, want = rec[f"grad_s{s}"], rec[f"ref_s{s}"]
            assert ef.same_bits(got, want), (s, int((got != want).sum()))
            assert got.tobytes() == recs[0][f"grad_s{s}"].tobytes(), s
        # sync(max_norm) is sync() then the clip restatement: the norm too
        assert bool(rec["clipped_s2"]) and not bool(rec["clipped_s3"])
        for s in (2, 3):
            got, want = rec[f"norm_s{s}"]
            assert got.tobytes() == want.tobytes(), s
        calls = [str(c) for c in rec["calls"]]
        nb = len(counts)
        enc, red = ("gather_q8_ef", "q8_reduce_ef") if feedback else ("gather_q8", "q8_reduce")
        assert calls.count(enc) == nb * STEPS and calls.count(red) == nb * STEPS
        assert calls.count("unpack_avg_q8") == nb * STEPS
        assert calls.count("norm_finish") == 2 and calls.count("scale_by") == 2
        other = ("gather_q8", "q8_reduce") if feedback else ("gather_q8_ef", "q8_reduce_ef")
        assert not [c for c in calls if c in other + ("grad_sumsq", "unpack_avg")]


@pytest.mark.parametrize("world", [2, 3])
def test_error_feedback_state_round_trips(world):
    for rec in _run(world, True):
        assert ef.same_bits(rec["encode"], rec["ref_encode"]) and rec["encode"].any()
        assert rec["reduce"].tobytes() == rec["ref_reduce"].tobytes() and rec["reduce"].any()
        assert bool(rec["reset"]) and bool(rec["round_trip"]) and bool(rec["mismatch_raises"])


@pytest.mark.parametrize("feedback", [False, True])
def test_dpsync_takes_the_wire_from_its_knobs(feedback):
    recs = _run(2, feedback)
    for rec in recs:
        assert bool(rec["dp_q8"])
        assert ef.same_bits(rec["dp_grad"], rec["dp_ref"])
        assert rec["dp_grad"].tobytes() == recs[0]["dp_grad"].tobytes()
        calls = [str(c) for c in rec["dp_calls"]]
        assert ("gather_q8_ef" if feedback else "gather_q8") in calls
        assert "unpack_avg_q8" in calls and "gather" not in calls
        default = [str(c) for c in rec["dp_default_calls"]]
        assert default and not [c for c in default if "q8" in c]
