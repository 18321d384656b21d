"""The 4-bit (MXFP4) wire, without a GPU.

1. The codec's restatement (tests/fp4_restatement.py) keeps its promises over chunk lengths 1, 31,
   32, 33, 4095 and 4096 (tails that are no multiple of 4 and of 32): the error bound
   |x - deq| <= 2^(E-127), the scale bound 2^(E-127) < amax/3 (E > 0), the identity of
   re-encoding decoded values, the tie table, groups at E = 0, 1 and 253, NaN and Inf groups,
   no nibble 8 anywhere, all-zero padding slots.
   The bounds are the codec's own: the scale is the smallest power of two with amax·2^-e <= 6,
   so amax·2^-e > 3 (E > 0) and neighbouring grid points are at most 2 apart (4 and 6): the
   nearest one is within 1. Nothing is measured from the code under test.
2. The C-ABI declares the four entry points, the Python binding types them, and argument errors
   are raised before any device work.
3. The knobs: error_feedback is accepted with wire="fp4"; DILOCO_OUTER_FP4_EF is read for the
   fp4 wire only; with the wire left at its default no fp4 kernel is called.
4. Two gloo CPU ranks through the reference's four calls on the checker backend
   (tests/fp4_oracle_kernels.py), Nesterov SGD and fused AdamW, error feedback on and off: θ,
   inner, .grad and the residuals equal the exchange composed by hand (Fp4Exchange) bit for
   bit, and both ranks hold byte-identical averaged slots."""
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

import fp4_restatement as fp4
from conftest import PKG, REPO
from diloco_amd import _lib

F = np.float32
LENGTHS = [1, 31, 32, 33, 4095, 4096]


def _wild(length, seed):
    """Magnitudes log-uniform over 1e-44 .. 1e38 (denormals included), random signs, zeros and
    negative zeros planted."""
    rng = np.random.default_rng(seed)
    x = (10.0 ** rng.uniform(-44, 38, length) * rng.choice([-1.0, 1.0], length)).astype(F)
    x[rng.random(length) < 0.1] = 0.0
    x[rng.random(length) < 0.05] = -0.0
    return x


def _groupwise(length, seed):
    """Every group of 32 at its own magnitude, elements within a factor 100 of each other, so
    most of them survive quantisation."""
    rng = np.random.default_rng(seed)
    g = -(-length // 32)
    mag = np.repeat(10.0 ** rng.uniform(-44, 36, g), 32)[:length]
    x = (mag * rng.uniform(0.01, 1.0, length) * rng.choice([-1.0, 1.0], length)).astype(F)
    x[rng.random(length) < 0.05] = 0.0
    return x


def _nibbles(slot):
    pay = slot[fp4.N_GROUPS:]
    return np.concatenate([pay & 15, pay >> 4])


def _scales(slot, n):
    with np.errstate(all="ignore"):
        return np.ldexp(1.0, np.repeat(slot[:fp4.N_GROUPS].astype(np.int64), 32) - 127)[:n]


@pytest.mark.parametrize("make", [_wild, _groupwise])
@pytest.mark.parametrize("length", LENGTHS)
def test_codec_properties(length, make):
    x = make(length, 100 + length)
    slot = fp4.encode_values(x)
    assert slot.shape == (fp4.SLOT,) and fp4.SLOT == 2176 == _lib.FP4_SLOT_BYTES
    e = slot[:fp4.N_GROUPS]
    assert e.max() <= 253
    deq = fp4.decode_slot(slot, length)
    assert np.isfinite(deq).all()
    s = _scales(slot, length)
    err = np.abs(x.astype(np.float64) - deq.astype(np.float64))
    assert (err <= s).all()
    pad = np.zeros(fp4.CHUNK, dtype=F)
    pad[:length] = x
    amax = np.abs(pad).reshape(-1, 32).max(axis=1).astype(np.float64)
    live = e > 0
    assert (np.ldexp(1.0, e[live].astype(np.int64) - 127) < amax[live] / 3).all()
    # nothing saturates: the largest element of a group is within the grid
    assert (amax <= 6 * np.ldexp(1.0, e.astype(np.int64) - 127)).all()
    # re-encoding decoded values is the identity (so the one-peer reduce is)
    again = fp4.decode_slot(fp4.encode_values(deq), length)
    assert again.tobytes() == deq.tobytes()
    assert not (_nibbles(slot) == 8).any()
    # elements past the length count as +0: their nibbles, and the scales of groups wholly past it
    assert not _nibbles(slot).reshape(2, -1).T.reshape(-1)[length:].any()
    assert not e[-(-length // 32):].any()
    assert (np.signbit(deq) == (np.signbit(x) & (deq != 0))).all()


def test_tie_table():
    """A group whose amax is 6 has E = 127 (scale 1): y = |x|. Ties go to the even code."""
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    want = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    x = np.array([6.0] + ties + [-t for t in ties], dtype=F)
    slot = fp4.encode_values(x)
    assert slot[0] == 127
    deq = fp4.decode_slot(slot, x.size)
    assert deq.tolist() == [6.0] + want + [-w for w in want]
    assert not (_nibbles(slot) == 8).any()  # -0.25 -> +0
    # one ulp to either side of a tie leaves it
    up = np.nextafter(np.array(ties, dtype=F), F(10))
    down = np.nextafter(np.array(ties, dtype=F), F(0))
    got_up = fp4.decode_slot(fp4.encode_values(np.concatenate([[F(6)], up])), 8)[1:]
    got_down = fp4.decode_slot(fp4.encode_values(np.concatenate([[F(6)], down])), 8)[1:]
    assert got_up.tolist() == [0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    assert got_down.tolist() == [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0]


def test_scale_rule_at_its_boundaries():
    """m <= 0.75 takes e = k - 3 (amax·2^-e in (4, 6]), above it e = k - 2 ((3, 4))."""
    for amax, want in [(6.0, 127), (np.nextafter(F(6), F(7)), 128), (4.0, 127),
                       (np.nextafter(F(4), F(0)), 127), (np.nextafter(F(3), F(4)), 127),
                       (3.0, 126), (1.0, 125), (8.0, 128)]:
        assert fp4.encode_values(np.array([amax], dtype=F))[0] == want, amax


def test_groups_at_the_ends_of_the_scale_range():
    two = lambda k: F(np.ldexp(1.0, k))  # noqa: E731
    x = np.zeros(96, dtype=F)
    # E = 0: amax 2^-126 and below clamps to the scale 2^-127; 2^-128, a denormal, survives
    x[0:4] = [two(-126), two(-128), -two(-127), two(-149)]
    # E = 1: amax = 6·2^-126
    x[32:35] = [F(6) * two(-126), -two(-126), two(-127)]
    # E = 253: amax = 3.25·2^126 (m = 0.8125 > 0.75, k = 128)
    x[64:67] = [F(3.25) * two(126), -two(126), two(125)]
    slot = fp4.encode_values(x)
    assert slot[:3].tolist() == [0, 1, 253]
    deq = fp4.decode_slot(slot, 96)
    assert deq[0:4].tolist() == [two(-126), two(-128), -two(-127), 0.0]
    assert deq[32:35].tolist() == [F(6) * two(-126), -two(-126), two(-127)]
    assert deq[64:67].tolist() == [F(3) * two(126), -two(126), two(125)]
    assert np.isfinite(deq).all()
    # a denormal amax is a value like any other
    d = np.array([two(-149), two(-140)], dtype=F)
    assert fp4.encode_values(d)[0] == 0 and not fp4.decode_slot(fp4.encode_values(d), 2).any()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_value_takes_exactly_its_group(bad):
    x = _groupwise(4096, 7)
    x[5 * 32 + 9] = bad
    slot = fp4.encode_values(x)
    assert slot[5] == 255 and (slot[:fp4.N_GROUPS] == 255).sum() == 1
    assert not slot[fp4.N_GROUPS + 5 * 16:fp4.N_GROUPS + 6 * 16].any()  # all 32 nibbles 0
    deq = fp4.decode_slot(slot)
    nan = np.isnan(deq)
    assert nan[160:192].all() and nan.sum() == 32
    _, r = fp4.quantise_with_residual(x)
    assert np.isnan(r[160:192]).all() and np.isfinite(np.delete(r, np.s_[160:192])).all()
    # through the reduce: NaN stays NaN in its group, position for position
    out, _ = fp4.reduce_slots(np.concatenate([slot, fp4.encode_values(x[:10])]), 2, 1, 2)
    assert np.array_equal(np.isnan(fp4.decode_slot(out)), nan)


def test_padding_slots_are_all_zero():
    zero = np.zeros(fp4.SLOT, dtype=np.uint8)
    assert fp4.encode_values(np.zeros(0, dtype=F)).tobytes() == zero.tobytes()
    assert fp4.encode_values(np.array([0.0, -0.0], dtype=F)).tobytes() == zero.tobytes()
    assert not fp4.decode_slot(zero).any() and not np.signbit(fp4.decode_slot(zero)).any()
    out, res = fp4.reduce_slots(np.zeros(3 * 2 * fp4.SLOT, dtype=np.uint8), 3, 2, 3,
                                np.zeros(2 * fp4.CHUNK, dtype=F))
    assert not out.any() and not res.any()


def test_one_peer_reduce_is_the_identity_on_decoded_values():
    x = _groupwise(4096, 11)
    slot = fp4.encode_values(x)
    for divisor in (1,):
        out, _ = fp4.reduce_slots(slot, 1, 1, divisor)
        assert fp4.decode_slot(out).tobytes() == fp4.decode_slot(slot).tobytes()


def test_error_feedback_carries_the_rounding_error():
    """x = d + r; r' = x - deq: what was sent plus the residual is what was asked for, up to the
    fp32 rounding of d + r and x - deq (each within 2^-24 of a value below 2·amax)."""
    d = _groupwise(4096, 13)
    r = np.zeros_like(d)
    sent = np.zeros(d.size, dtype=np.float64)
    T = 16
    for _ in range(T):
        slot, r = fp4.encode_chunk(d, np.zeros_like(d), r)
        sent += fp4.decode_slot(slot).astype(np.float64)
    amax = np.repeat(np.abs(d).reshape(-1, 32).max(axis=1), 32).astype(np.float64)
    assert (np.abs(sent + r - T * d.astype(np.float64)) <= T * 4 * 2.0 ** -24 * 2 * amax).all()


@pytest.mark.parametrize("row", ["delta_fp4_ef", "unpack_adamw_fp4", "fp4_reduce_ef"])
def test_reference_stays_inside_its_footprint(row):
    """The CPU stand-ins that tests/test_fp4_gpu.py compares the kernels' footprints with write
    nothing outside the documented outputs themselves (both sentinels, the mixed placement)."""
    import fp4_footprint as f4

    flat = row in f4.FLAT_ROWS
    for case in (f4.FLAT_ROWS if flat else f4.TREE_ROWS)[row]():
        if flat:
            f4.run_flat_case(case)
        else:
            f4.run_case(case, places=case.places[2:])


# ---- the C-ABI -------------------------------------------------------------------------------
ENTRY_POINTS = (("dl_delta_fp4", 7), ("dl_fp4_reduce", 7), ("dl_unpack_sgd_fp4", 11),
                ("dl_unpack_adamw_fp4", 15))


def test_abi_declares_the_fp4_entry_points():
    with open(os.path.join(REPO, "include", "diloco_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+DL_FP4_SLOT_BYTES\s+2176\b", header)
    lib = _lib.load()
    for name, nargs in ENTRY_POINTS:
        assert re.search(r"DL_API\s+int\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(lib, name)


def test_argument_checks_come_before_the_device():
    E = _lib.DilocoHipError
    with pytest.raises(E, match="null tree"):
        _lib.call("dl_delta_fp4", None, 0, 0, 64, None, 192, None)
    with pytest.raises(E, match="null tree"):
        _lib.call("dl_unpack_sgd_fp4", None, 0, 64, 128, 192, 0.7, 0.9, 1, 0, 0, None)
    with pytest.raises(E, match="null tree"):
        _lib.call("dl_unpack_adamw_fp4", None, 0, 64, 128, 192, 256, 1.0, 0.1, 0.95, 0.05, -0.1,
                  1.0, 1e-8, 0, None)
    with pytest.raises(E, match="recv is null") as e:
        _lib.call("dl_fp4_reduce", None, 1, 1, 1, None, 128, None)
    assert e.value.code == -1 and "dl_fp4_reduce" in str(e.value)  # DL_E_ARG
    with pytest.raises(E, match="residual not 16-B aligned") as e:
        _lib.call("dl_fp4_reduce", 64, 1, 1, 1, 68, 128, None)
    assert e.value.code == -3  # DL_E_ALIGN
    with pytest.raises(E, match="out not 16-B aligned"):
        _lib.call("dl_fp4_reduce", 64, 1, 1, 1, None, 136, None)
    with pytest.raises(E, match="in place needs n_peers == 1"):
        _lib.call("dl_fp4_reduce", 64, 2, 1, 2, None, 64, None)
    for n, m, div in [(0, 1, 1), (1, -1, 1), (1, 1, 0)]:
        with pytest.raises(E, match="dl_fp4_reduce: n"):
            _lib.call("dl_fp4_reduce", 64, n, m, div, None, 128, None)


# ---- the knobs -------------------------------------------------------------------------------
def _inner_model():
    m = torch.nn.Module()
    m.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(8))])
    return m


def test_fp4_is_an_outer_wire_and_takes_error_feedback(monkeypatch):
    from diloco_amd.mirror import OUTER_WIRES
    from diloco_amd.utils import _Q8_EF, _WIRE, get_outer_model

    assert "fp4" in OUTER_WIRES
    for v in ("DILOCO_OUTER_WIRE", "DILOCO_OUTER_FP4_EF", "DILOCO_OUTER_Q8_EF"):
        monkeypatch.delenv(v, raising=False)
    o = get_outer_model(_inner_model(), wire="fp4", error_feedback=True)
    assert getattr(o, _WIRE) == "fp4" and getattr(o, _Q8_EF) is True
    assert getattr(get_outer_model(_inner_model(), wire="fp4"), _Q8_EF) is False  # default off
    # each variable is consulted for its own wire only
    monkeypatch.setenv("DILOCO_OUTER_Q8_EF", "1")
    assert getattr(get_outer_model(_inner_model(), wire="fp4"), _Q8_EF) is False
    monkeypatch.setenv("DILOCO_OUTER_FP4_EF", "1")
    monkeypatch.delenv("DILOCO_OUTER_Q8_EF")
    assert getattr(get_outer_model(_inner_model(), wire="fp4"), _Q8_EF) is True
    assert getattr(get_outer_model(_inner_model(), wire="int8"), _Q8_EF) is False
    assert getattr(get_outer_model(_inner_model(), wire="f32"), _Q8_EF) is False
    monkeypatch.setenv("DILOCO_OUTER_WIRE", "fp4")
    assert getattr(get_outer_model(_inner_model()), _WIRE) == "fp4"
    with pytest.raises(ValueError, match="sync"):  # as the other narrow wires
        get_outer_model(_inner_model(), wire="fp4", write_back="sync")


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


def _worker(rank, world, port, rule, wire, feedback, out):
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
              "DILOCO_OUTER_Q8_EF", "DILOCO_OUTER_FP4_EF"):
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
    from fp4_oracle_kernels import Fp4OracleKernels
    from oracle import oracle

    k = Fp4OracleKernels()
    kernels.set_default_kernels(k)
    world_ = World.from_default_group(1)
    spec = get_tree("micro")
    numels = spec.numels()
    shapes = [s for _, s in spec.params()]
    theta0 = synth.outer_tree(numels, spec.init_spec())
    inner = torch.nn.Module()
    inner.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(v.copy()).view(s))
                                       for v, s in zip(theta0, shapes)])
    kw = {} if wire is None else dict(wire=wire, error_feedback=feedback)
    outer = get_outer_model(inner, placement="device", **kw)
    rec = {}
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
    ex = fp4.Fp4Exchange(numels, counts, world, ef=feedback)

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
        if wire != "fp4":
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
        S = dev._q8["S"]
        rec[f"slots_s{s}"] = np.concatenate(
            [dev._q8["slots"][base * S:(base + nch) * S].numpy().copy()
             for nch, _m, base, _rb in dev._q8["plan"]])
        rec[f"ref_slots_s{s}"] = np.concatenate(ex.avg_slots)
        rec[f"grad_s{s}"] = _host([p.grad for p in outer.parameters()])  # decoded when read
        rec[f"ref_grad_s{s}"] = np.concatenate(avg)

    for s in range(1, STEPS + 1):
        outer_step(s)
    st = q8_error_feedback_state(outer)
    rec["state_is_none"] = np.array(st is None)
    if wire == "fp4" and feedback:
        rec["encode"] = st["encode"].numpy()
        rec["ref_encode"] = np.zeros(dev.tree.total, dtype=F)
        for t, o in enumerate(dev.offs):
            rec["ref_encode"][o:o + numels[t]] = ex.enc[rank][t]
        rec["reduce"] = np.concatenate([a.numpy() for a in st["reduce"]])
        rec["ref_reduce"] = np.concatenate([ex.red[b][rank] for b in range(len(counts))])
        # the state leaves, is reset, comes back, and the next step continues as if untouched
        load_q8_error_feedback_state(outer, None)
        z = q8_error_feedback_state(outer)
        rec["reset"] = np.array(not z["encode"].any() and not any(a.any() for a in z["reduce"]))
        load_q8_error_feedback_state(outer, st)
        outer_step(STEPS + 1)
    rec["calls"] = np.array([c[0] for c in k.calls])
    rec["ef_calls"] = np.array([bool(c[2]) for c in k.calls
                                if c[0] in ("delta_fp4", "fp4_reduce")])
    np.savez(os.path.join(out, f"r{rank}.npz"), **rec)
    dist.barrier()
    dist.destroy_process_group()


def _run(rule, wire="fp4", feedback=True, world=2):
    out = tempfile.mkdtemp(prefix="dl_fp4_")
    # forked workers, as tests/test_dist_gloo.py: CPU only, no HIP state to inherit
    mp.start_processes(_worker, args=(world, _free_port(), rule, wire, feedback, out),
                       nprocs=world, join=True, start_method="fork")
    return [dict(np.load(os.path.join(out, f"r{r}.npz"))) for r in range(world)]


@pytest.mark.parametrize("feedback", [True, False])
@pytest.mark.parametrize("rule", ["sgd", "adamw"])
def test_four_calls_on_the_fp4_wire_match_the_restatement(rule, feedback):
    recs = _run(rule, feedback=feedback)
    for rec in recs:
        nb = int(rec["n_buckets"])
        assert nb >= 2
        steps = STEPS + (1 if feedback else 0)
        calls = [str(c) for c in rec["calls"]]
        assert calls.count("delta_fp4") == calls.count("fp4_reduce") == nb * steps
        assert calls.count("unpack_adamw_fp4" if rule == "adamw" else "unpack_sgd_fp4") == nb * steps
        assert not [c for c in calls if "q8" in c]
        assert (rec["ef_calls"] == feedback).all()
        for s in range(1, steps + 1):
            want = rec[f"ref_theta_s{s}"]
            assert fp4.same_bits(rec[f"theta_s{s}"], want), s
            assert fp4.same_bits(rec[f"inner_s{s}"], want), s
            assert fp4.same_bits(rec[f"grad_s{s}"], rec[f"ref_grad_s{s}"]), s
            assert rec[f"slots_s{s}"].tobytes() == rec[f"ref_slots_s{s}"].tobytes(), s
            assert rec[f"slots_s{s}"].tobytes() == recs[0][f"slots_s{s}"].tobytes(), s
            assert rec[f"theta_s{s}"].tobytes() == recs[0][f"theta_s{s}"].tobytes(), s
            assert rec[f"slots_s{s}"].any()
        assert bool(rec["state_is_none"]) == (not feedback)
        if feedback:
            assert rec["encode"].tobytes() == rec["ref_encode"].tobytes()
            assert rec["reduce"].tobytes() == rec["ref_reduce"].tobytes()
            assert rec["encode"].any() and rec["reduce"].any()
            assert bool(rec["reset"])


def test_default_wire_calls_no_fp4_kernel():
    for rec in _run("adamw", wire=None):  # the AdamW stand-ins log their calls
        calls = [str(c) for c in rec["calls"]]
        assert calls and not [c for c in calls if "fp4" in c]
