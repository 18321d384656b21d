"""Error feedback on the int8 wire, without a GPU.

1. What the restatement (tests/q8_ef_restatement.py) promises over 64 outer steps of a constant
   pseudo-gradient d with one element of 1.0 and ~1e-3 elsewhere: the residual stays within
   half a quantisation step, nothing is lost (Σ deq + r = T·d up to fp32 rounding), and what was
   transmitted is within half a step of T·d -- a bound the plain quantiser misses by far.
   The fp32 slack T·4·2^-23·amax: each step rounds d + r, float(q)·s and x - q·s once each
   (3 roundings of values <= amax·(1 + 1/254)), summed over T steps.
2. The C-ABI declares both entry points and the Python binding types them (ABI version 8).
3. The knobs: error_feedback needs the int8 wire; off means no _ef kernel is ever called.
4. Two gloo CPU ranks through the reference's four calls on the checker backend
   (tests/q8_ef_oracle_kernels.py), SGD Nesterov and fused AdamW: θ equal on both ranks and
   equal to the exchange composed by hand (EFExchange); the state helpers round-trip."""
import os
import re
import socket
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import q8_ef_restatement as ef
from conftest import PKG, REPO
from diloco_amd import _lib
from oracle import oracle

F = np.float32
T = 64
EPS = 4 * 2.0 ** -23


def _chunk(length):
    rng = np.random.default_rng(1234 + length)
    d = (1e-3 * rng.standard_normal(length)).astype(F)
    d[length // 2] = 1.0
    return d


@pytest.mark.parametrize("length", [1, 5, 257, 4095, 4096])
def test_restatement_carries_the_rounding_error(length):
    d = _chunk(length)
    zero = np.zeros(length, dtype=F)
    r = zero.copy()
    sent = np.zeros(length, dtype=np.float64)
    plain = np.zeros(length, dtype=np.float64)
    smax = amax = 0.0
    for _ in range(T):
        x = (d + r).astype(F)
        slot, r = ef.encode_chunk(d, zero, r)
        s = float(slot[:4].view(F)[0])
        assert np.abs(r).max() <= 0.5 * s * (1 + 1e-6)
        sent += oracle.q8_deq(slot, length).astype(np.float64)
        plain += oracle.q8_deq(oracle.delta_q8_from(d), length).astype(np.float64)
        smax, amax = max(smax, s), max(amax, float(np.abs(x).max()))
    want = T * d.astype(np.float64)
    slack = T * EPS * amax
    assert np.abs(sent + r - want).max() <= slack
    err = np.abs(sent - want).max()
    print(f"len {length}: error feedback {err:.4g}, plain {np.abs(plain - want).max():.4g}, "
          f"bound {0.5 * smax + slack:.4g}")
    assert err <= 0.5 * smax + slack
    if length > 1:  # a chunk of one element has no small neighbour to lose
        assert np.abs(plain - want).max() > 0.5 * smax + slack


def test_abi_declares_the_error_feedback_entry_points():
    with open(os.path.join(REPO, "include", "diloco_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+DL_ABI_VERSION\s+8\b", header)
    assert _lib.ABI_VERSION == 8
    for name, nargs in (("dl_delta_q8_ef", 7), ("dl_q8_reduce_ef", 7)):
        assert re.search(r"DL_API\s+int\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    lib = _lib.load()
    assert lib.dl_abi_version() == 8
    assert hasattr(lib, "dl_delta_q8_ef") and hasattr(lib, "dl_q8_reduce_ef")


def test_argument_checks_come_before_the_device():
    with pytest.raises(_lib.DilocoHipError, match="null tree"):
        _lib.call("dl_delta_q8_ef", None, 0, 0, 64, 128, 192, None)
    with pytest.raises(_lib.DilocoHipError, match="residual is null") as e:
        _lib.call("dl_q8_reduce_ef", 64, 1, 1, 1, None, 128, None)
    assert e.value.code == -1 and "dl_q8_reduce_ef" in str(e.value)  # DL_E_ARG
    with pytest.raises(_lib.DilocoHipError, match="residual not 16-B aligned") as e:
        _lib.call("dl_q8_reduce_ef", 64, 1, 1, 1, 68, 128, None)
    assert e.value.code == -3  # DL_E_ALIGN
    with pytest.raises(_lib.DilocoHipError, match="in place needs n_peers == 1"):
        _lib.call("dl_q8_reduce_ef", 64, 2, 1, 2, 256, 64, None)


def _inner_model():
    m = torch.nn.Module()
    m.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(8))])
    return m


@pytest.mark.parametrize("wire", ["f32", "bf16"])
def test_error_feedback_needs_the_int8_wire(wire, monkeypatch):
    from diloco_amd.outer import OuterSync
    from diloco_amd.utils import _Q8_EF, get_outer_model
    from q8_ef_oracle_kernels import Q8EFOracleKernels

    dtype = {"f32": torch.float32, "bf16": torch.bfloat16}[wire]
    with pytest.raises(ValueError, match="int8"):
        OuterSync([torch.zeros(8)], world_size=1, wire_dtype=dtype, error_feedback=True,
                  kernels=Q8EFOracleKernels())
    with pytest.raises(ValueError, match="int8"):
        get_outer_model(_inner_model(), wire=wire, error_feedback=True)
    # the variable is consulted for the int8 wire only
    monkeypatch.setenv("DILOCO_OUTER_Q8_EF", "1")
    assert getattr(get_outer_model(_inner_model(), wire=wire), _Q8_EF) is False


# ---- two gloo ranks through the four calls ---------------------------------------------------
SGD = dict(lr=0.7, momentum=0.9, nesterov=True)
ADAMW = dict(lr=0.01, betas=(0.9, 0.95), weight_decay=0.1)
STEPS = 3


class _Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _host(ts):
    return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in ts])


def _worker(rank, world, port, rule, feedback, out):
    for p in (PKG, REPO, os.path.join(REPO, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    torch.set_num_threads(1)
    import expect

    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      DILOCO_OUTER_BUCKET_ELEMS=str(expect.MICRO_Q8_CAP),
                      DILOCO_OUTER_ADAMW="fused", DILOCO_OUTER_FUSED="1")
    for v in ("DILOCO_OUTER_EXCHANGE", "DILOCO_DP_EXCHANGE", "DILOCO_OUTER_WIRE",
              "DILOCO_OUTER_Q8_EF"):
        os.environ.pop(v, None)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank,
                            world_size=world)
    from adamw_restatement import AdamWState
    from diloco_amd import kernels, synth
    from diloco_amd.comm import TrainingComm
    from diloco_amd.trees import get_tree
    from diloco_amd.utils import (compute_pseudo_gradient, get_optimizer, get_outer_model,
                                  load_q8_error_feedback_state, outer_mirror,
                                  q8_error_feedback_state, sync_inner_model)
    from diloco_amd.world import World
    from q8_ef_oracle_kernels import Q8EFOracleKernels

    k = Q8EFOracleKernels()
    kernels.set_default_kernels(k)
    world_ = World.from_default_group(1)
    spec = get_tree("micro")
    numels = spec.numels()
    shapes = [s for _, s in spec.params()]
    theta0 = synth.outer_tree(numels, spec.init_spec())
    inner = torch.nn.Module()
    inner.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(v.copy()).view(s))
                                       for v, s in zip(theta0, shapes)])
    outer = get_outer_model(inner, placement="device", wire="int8", error_feedback=feedback)
    rec = {}
    rec["state_before"] = np.array(q8_error_feedback_state(outer) is None)
    if rule == "sgd":
        opt = get_optimizer(outer, _Cfg(type="SGD", **SGD))
        theta = [t.copy() for t in theta0]
        buf = [np.empty_like(t) for t in theta]
    else:
        opt = get_optimizer(outer, _Cfg(type="AdamW", **ADAMW))
        ref = AdamWState(theta0, **ADAMW)
        theta = ref.theta
    comm = TrainingComm(world_, (1, 1, 32), None)
    dev = outer_mirror(outer)
    dev = getattr(dev, "dev", dev)
    counts = [c1 - c0 for c0, c1 in dev.tree.bucket_chunks]
    rec["n_buckets"] = np.array(len(counts))
    ex = ef.EFExchange(numels, counts, world)

    def outer_step(s):
        nonlocal theta
        vals = [synth.inner_tree(theta, s, r) for r in range(world)]
        with torch.no_grad():
            for p, v in zip(inner.parameters(), vals[rank]):
                p.copy_(torch.from_numpy(v).view(p.shape))
        compute_pseudo_gradient(inner, outer)
        comm.sync_gradients(outer)
        opt.step()
        sync_inner_model(outer, inner)
        if not feedback:
            return
        deltas = [[oracle.delta(t, i) for t, i in zip(theta, v)] for v in vals]
        avg = ex.average(deltas)
        if rule == "sgd":
            for t in range(len(theta)):
                oracle.sgd(theta[t], buf[t], avg[t], SGD["lr"], SGD["momentum"], True, s == 1)
        else:
            ref.step_grads(avg)
            theta = ref.theta
        rec[f"theta_s{s}"] = _host(outer.parameters())
        rec[f"inner_s{s}"] = _host(inner.parameters())
        rec[f"ref_theta_s{s}"] = np.concatenate(theta)

    for s in range(1, STEPS + 1):
        outer_step(s)
    rec["calls"] = np.array([c[0] for c in k.calls])
    if feedback:
        # the state leaves, is reset, comes back, and the next step continues as if untouched
        st = q8_error_feedback_state(outer)
        rec["encode"] = st["encode"].numpy()
        rec["ref_encode"] = np.zeros(dev.tree.total, dtype=F)
        for t, o in enumerate(dev.offs):
            rec["ref_encode"][o:o + numels[t]] = ex.enc[rank][t]
        rec["reduce"] = np.concatenate([a.numpy() for a in st["reduce"]])
        rec["ref_reduce"] = np.concatenate([ex.red[b][rank] for b in range(len(counts))])
        load_q8_error_feedback_state(outer, None)
        z = q8_error_feedback_state(outer)
        rec["reset"] = np.array(not z["encode"].any() and not any(a.any() for a in z["reduce"]))
        load_q8_error_feedback_state(outer, st)
        back = q8_error_feedback_state(outer)
        rec["round_trip"] = np.array(
            back["encode"].numpy().tobytes() == rec["encode"].tobytes()
            and all(a.numpy().tobytes() == b.numpy().tobytes()
                    for a, b in zip(back["reduce"], st["reduce"])))
        bad = dict(st, encode=st["encode"][:-1])
        try:
            load_q8_error_feedback_state(outer, bad)
            rec["mismatch_raises"] = np.array(False)
        except ValueError:
            rec["mismatch_raises"] = np.array(True)
        outer_step(STEPS + 1)
    np.savez(os.path.join(out, f"r{rank}.npz"), **rec)
    dist.barrier()
    dist.destroy_process_group()


def _run(rule, feedback=True, world=2):
    out = tempfile.mkdtemp(prefix="dl_q8_ef_")
    # forked workers, as tests/test_dist_gloo.py: CPU only, no HIP state to inherit
    mp.start_processes(_worker, args=(world, _free_port(), rule, feedback, out),
                       nprocs=world, join=True, start_method="fork")
    return [dict(np.load(os.path.join(out, f"r{r}.npz"))) for r in range(world)]


@pytest.mark.parametrize("rule", ["sgd", "adamw"])
def test_four_calls_with_error_feedback_match_the_restatement(rule):
    recs = _run(rule)
    for rec in recs:
        nb = int(rec["n_buckets"])
        assert nb >= 2
        assert bool(rec["state_before"])  # nothing built before the first exchange
        calls = [str(c) for c in rec["calls"]]
        assert calls.count("delta_q8_ef") == nb * STEPS
        assert calls.count("q8_reduce_ef") == nb * STEPS
        for s in range(1, STEPS + 2):
            want = rec[f"ref_theta_s{s}"]
            assert ef.same_bits(rec[f"theta_s{s}"], want), s
            assert ef.same_bits(rec[f"inner_s{s}"], want), s
            assert rec[f"theta_s{s}"].tobytes() == recs[0][f"theta_s{s}"].tobytes(), s
        assert rec["encode"].tobytes() == rec["ref_encode"].tobytes()
        assert rec["reduce"].tobytes() == rec["ref_reduce"].tobytes()
        assert rec["encode"].any() and rec["reduce"].any()
        assert bool(rec["reset"]) and bool(rec["round_trip"]) and bool(rec["mismatch_raises"])


def test_feature_off_calls_no_error_feedback_kernel():
    for rec in _run("sgd", feedback=False):
        assert not [c for c in rec["calls"] if str(c).endswith("_ef")]
