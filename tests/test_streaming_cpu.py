"""Streaming DiLoCo on the CPU: the schedule, the restated merge, and StreamingOuterSync on the
checker backend (tests/streaming_oracle_kernels.py) in one process and over gloo process groups,
against the numpy simulator of tests/streaming_restatement.py. Bit for bit except at four ranks,
where gloo's summation order is not rank order and the project's 1e-6 normwise bound applies."""
import os
import socket
import sys
import tempfile
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import streaming_restatement as sr
from adamw_restatement import F, libm_fmaf
from conftest import PKG, REPO, normwise_ok, split
from diloco_amd import synth
from diloco_amd.outer import OuterSync
from diloco_amd.streaming import StreamingOuterSync, fragment_events, split_buckets
from diloco_amd.trees import get_tree
from streaming_oracle_kernels import StreamingOracleKernels

CAP = 4096
HYPER = dict(lr=0.7, momentum=0.9, nesterov=True)
# (H, P, tau, alpha, pattern)
CASES = [(2, 1, 0, 0.0, "strided"), (4, 2, 1, 0.5, "strided"), (6, 3, 3, 0.3, "strided"),
         (6, 3, 3, 0.3, "sequential")]


def _theta0():
    spec = get_tree("micro")
    return synth.outer_tree(spec.numels(), spec.init_spec())


def _flat(ts):
    return np.concatenate([t.detach().float().numpy().reshape(-1) for t in ts])


def _engine(params, H, P, tau, alpha, pattern="strided", **kw):
    kw.setdefault("kernels", StreamingOracleKernels())
    kw.setdefault("world_size", 1)
    return StreamingOuterSync(params, sync_every=H, fragments=P, delay=tau, alpha=alpha,
                              pattern=pattern, bucket_cap_elems=CAP, **HYPER, **kw)


def _inner_step(params, rank, t):
    """The stand-in inner step on the engine's tensors."""
    for i, p in enumerate(params):
        p.add_(torch.from_numpy(sr.perturbation(rank, t, i, p.numel())).view(p.shape))


def _state(eng, params, wire=True):
    out = {"theta": _flat(eng.unpacked(eng.theta)), "mom": _flat(eng.unpacked(eng.mom)),
           "inner": _flat(params)}
    if wire:
        out["wire"] = _flat(eng.unpacked(eng.wire))
    return out


def _same(got, sim, what, rank=0):
    for k, v in got.items():
        assert v.tobytes() == sim.flat(k, rank).tobytes(), (what, k, int((v != sim.flat(k, rank)).sum()))


# ---- the schedule -----------------------------------------------------------------------------
@pytest.mark.parametrize("H,P,tau", [(4, 1, 0), (4, 2, 1), (6, 3, 3), (8, 4, 7)])
def test_fragment_events(H, P, tau):
    begins = {p: [] for p in range(P)}
    finishes = {p: [] for p in range(P)}
    open_, most = set(), 0
    for t in range(1, 3 * H + 1):
        finish, begin = fragment_events(t, H, P, tau)
        # begins are at distinct residues and every finish is tau after its begin
        assert len(begin) <= 1 and len(finish) <= 1
        for p in finish:
            if tau:
                assert p in open_
                open_.discard(p)
            finishes[p].append(t)
        for p in begin:
            assert p not in open_  # never two exchanges of one fragment open
            begins[p].append(t)
            if tau:
                open_.add(p)
        most = max(most, len(open_))
    residues = set()
    for p in range(P):
        assert [t % H for t in begins[p]] == [begins[p][0] % H] * len(begins[p])
        assert np.diff(begins[p]).tolist() == [H] * (len(begins[p]) - 1) and len(begins[p]) == 3
        residues.add(begins[p][0] % H)
        assert begins[p][0] == (p + 1) * (H // P)
        assert finishes[p] == [t + tau for t in begins[p] if t + tau <= 3 * H]
    assert len(residues) == P
    if (H, P, tau) in ((6, 3, 3), (8, 4, 7)):
        assert most >= 2
    if P == 1:  # the classic schedule
        assert begins[0] == [H, 2 * H, 3 * H]


@pytest.mark.parametrize("args", [(1, 4, 3, 0), (1, 4, 2, 4), (1, 4, 2, -1), (0, 4, 2, 1),
                                  (1, 4, 0, 0), (1, 6, 3, 6)])
def test_fragment_events_bad_arguments(args):
    with pytest.raises(ValueError):
        fragment_events(*args)


def test_split_buckets():
    assert split_buckets(7, 3, "strided") == [[0, 3, 6], [1, 4], [2, 5]]
    assert split_buckets(7, 3, "sequential") == [[0, 1, 2], [3, 4], [5, 6]]
    assert split_buckets(12, 1, "sequential") == [list(range(12))]
    with pytest.raises(ValueError, match="bucket_cap_elems"):
        split_buckets(2, 3, "strided")
    for P in (1, 2, 3, 5):
        for pattern in ("strided", "sequential"):
            assert split_buckets(11, P, pattern) == sr.fragments_of(11, P, pattern)


# ---- the restated merge ------------------------------------------------------------------------
def test_merge_restatement_against_libm():
    """merge(x, th, alpha) == fmaf(alpha, fl(x - th), th) of libm, on 10^4 random triples over
    many decades and on the special values."""
    rng = np.random.default_rng(5)
    n = 10000
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-20, 20, n)).astype(F)
    th = (rng.standard_normal(n) * 10.0 ** rng.uniform(-20, 20, n)).astype(F)
    near = rng.random(n) < 0.5  # half of them close together, where the subtract cancels
    th[near] = (x[near] * (1 + rng.standard_normal(near.sum()) * 1e-6)).astype(F)
    a = rng.random(n).astype(F)
    fmax, den = np.finfo(F).max, F(1e-42)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, den, -den, fmax, -fmax, 1.0], F)
    sx, sth, sa = np.meshgrid(special, special, np.array([0.0, 0.3, 0.5, 0.99], F))
    x, th, a = (np.concatenate([u, v.reshape(-1)]) for u, v in ((x, sx), (th, sth), (a, sa)))
    fm = libm_fmaf()
    with np.errstate(all="ignore"):
        d = (x - th).astype(F)
        got = sr.merge(x, th, a)
    want = np.array([fm(float(a[i]), float(d[i]), float(th[i])) for i in range(x.size)], F)
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all()
    assert got[~nan].tobytes() == want[~nan].tobytes()


@pytest.mark.parametrize("row", ["unpack_sgd_merge", "unpack_adamw_merge"])
def test_merge_reference_stays_inside_its_footprint(row):
    """The CPU stand-ins that tests/test_streaming_gpu.py compares the kernels' bytes with write
    no padding, no guard band, not the wire and, in a single-bucket call, no other bucket."""
    import streaming_footprint as sfp

    for wire in ("f32", "bf16"):
        for case in sfp.TREE_ROWS[row](wire):
            sfp.run_case(case, places=sfp.fpt.PLACES[2:])


# ---- the engine, one process ---------------------------------------------------------------------
def test_micro_tree_has_twelve_buckets():
    assert len(sr.bucket_segments(get_tree("micro").numels(), CAP)) == 12


@pytest.mark.parametrize("H,P,tau,alpha,pattern", CASES)
def test_engine_matches_the_simulator(H, P, tau, alpha, pattern):
    theta0 = _theta0()
    params = [torch.from_numpy(t.copy()) for t in theta0]
    eng = _engine(params, H, P, tau, alpha, pattern)
    sim = sr.StreamSim(theta0, 1, H, P, tau, alpha, CAP, pattern, **HYPER)
    assert eng.tree.n_buckets == 12 and eng.fragment_buckets == sim.frags
    with pytest.raises(RuntimeError, match="after_inner_step"):
        eng.step()
    seen_open = 0
    for t in range(1, 2 * H + 2):
        _inner_step(params, 0, t)
        sim.inner_steps()
        eng.after_inner_step()
        sim.after_inner_step()
        assert eng.in_flight == list(sim.open) and eng.bucket_steps == sim.bucket_steps
        seen_open = max(seen_open, len(eng.in_flight))
        _same(_state(eng, params), sim, (H, P, tau, t))
    assert seen_open == (0 if tau == 0 else 2 if (H, P, tau) == (6, 3, 3) else 1)
    eng.flush()
    sim.flush()
    assert eng.in_flight == [] and eng.inner_steps == 2 * H + 1
    _same(_state(eng, params), sim, "flush")
    eng.close()


def test_classic_schedule_is_the_plain_outer_step():
    """(P = 1, tau = 0, alpha = 0): after every H-th call the state is bit-identical to a plain
    OuterSync(shard=False) stepped at those steps on the same inner trajectory."""
    H = 2
    theta0 = _theta0()
    pa = [torch.from_numpy(t.copy()) for t in theta0]
    pb = [torch.from_numpy(t.copy()) for t in theta0]
    a = _engine(pa, H, 1, 0, 0.0)
    b = OuterSync(pb, shard=False, world_size=1, bucket_cap_elems=CAP,
                  kernels=StreamingOracleKernels(), **HYPER)
    for t in range(1, 3 * H + 1):
        _inner_step(pa, 0, t)
        _inner_step(pb, 0, t)
        a.after_inner_step()
        if t % H == 0:
            b.step()
            for x, y in ((a.theta, b.theta), (a.mom, b.mom)):
                assert torch.equal(x, y)
            assert _flat(pa).tobytes() == _flat(pb).tobytes()
            assert _flat(pa).tobytes() == _flat(a.unpacked(a.theta)).tobytes()  # inner = θ
    assert a.steps_done == b.steps_done == 3
    a.close()
    b.close()


# ---- checkpoint ------------------------------------------------------------------------------------
def test_checkpoint_resume_is_bit_exact():
    H, P, tau, alpha = 4, 2, 1, 0.5
    theta0 = _theta0()
    pa = [torch.from_numpy(t.copy()) for t in theta0]
    a = _engine(pa, H, P, tau, alpha)
    m, k = 6, 7  # 6: fragment 0 began at t = 6 and is in flight
    for t in range(1, m + 1):
        _inner_step(pa, 0, t)
        a.after_inner_step()
    assert a.in_flight == [0]
    with pytest.raises(RuntimeError, match="flush"):
        a.state_dict()
    a.flush()
    st = a.state_dict()
    assert st["bucket_steps"] == a.bucket_steps and st["steps"] == min(a.bucket_steps)
    assert len(set(st["bucket_steps"])) == 2  # the fragments are at different step counts
    assert (st["inner_steps"], st["sync_every"], st["fragments"], st["delay"], st["alpha"]) == (
        m, H, P, tau, alpha)
    pb = [p.clone() for p in pa]  # the inner model's own checkpoint
    b = _engine(pb, H, P, tau, alpha)
    b.load_state_dict(st)
    assert _flat(pb).tobytes() == _flat(pa).tobytes()  # the merged inner is not overwritten
    for t in range(m + 1, m + k + 1):
        for params, eng in ((pa, a), (pb, b)):
            _inner_step(params, 0, t)
            eng.after_inner_step()
        assert a.in_flight == b.in_flight
    a.flush()
    b.flush()
    sa, sb = _state(a, pa), _state(b, pb)
    for key in sa:
        assert sa[key].tobytes() == sb[key].tobytes(), key
    assert a.bucket_steps == b.bucket_steps and a.inner_steps == b.inner_steps == m + k
    # another bucket layout is refused
    c = StreamingOuterSync([p.clone() for p in pa], sync_every=H, fragments=P, delay=tau,
                           alpha=alpha, bucket_cap_elems=3 * CAP, world_size=1,
                           kernels=StreamingOracleKernels(), **HYPER)
    assert c.tree.n_buckets != a.tree.n_buckets
    with pytest.raises(ValueError, match="bucket"):
        c.load_state_dict(st)
    for e in (a, b, c):
        e.close()


# ---- constructor refusals ------------------------------------------------------------------------
@pytest.mark.parametrize("kw,word", [
    (dict(wire_dtype=torch.int8), "int8"), (dict(shard=True), "shard"),
    (dict(exchange="a2a"), "a2a"), (dict(wire_dtype=torch.int8, error_feedback=True), "int8"),
    (dict(error_feedback=True), "error_feedback"),
    (dict(fragments=13), "bucket_cap_elems"), (dict(sync_every=13, fragments=2), "multiple"),
    (dict(delay=4), "delay"), (dict(delay=7), "delay"), (dict(alpha=1.0), "alpha"),
    (dict(alpha=-0.1), "alpha"), (dict(alpha=float("nan")), "alpha"),
    (dict(pattern="random"), "pattern")])
def test_constructor_refusals(kw, word):
    args = dict(sync_every=4, fragments=2, delay=1, alpha=0.5, bucket_cap_elems=CAP, world_size=1,
                kernels=StreamingOracleKernels())
    if "fragments" in kw and "sync_every" not in kw:
        args["sync_every"] = 13 * 4
    args.update(kw)
    params = [torch.from_numpy(t.copy()) for t in _theta0()]
    with pytest.raises(ValueError, match=word):
        StreamingOuterSync(params, **args)


# ---- gloo process groups ---------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, case, wire, steps, out):
    for p in (PKG, REPO, os.path.join(REPO, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank,
                            world_size=world)
    H, P, tau, alpha = case
    params = [torch.from_numpy(t.copy()) for t in _theta0()]
    eng = _engine(params, H, P, tau, alpha, world_size=world, rank=rank,
                  wire_dtype=torch.bfloat16 if wire == "bf16" else torch.float32)
    assert not eng._local()
    rec = {}
    for t in range(1, steps + 1):
        _inner_step(params, rank, t)
        eng.after_inner_step()
        for k, v in _state(eng, params, wire=False).items():  # the wire is the collective's
            rec[f"{k}_t{t}"] = v                               # while an exchange is in flight
    eng.flush()
    for k, v in _state(eng, params).items():
        rec[f"{k}_end"] = v
    np.savez(os.path.join(out, f"r{rank}.npz"), **rec)
    dist.barrier()
    dist.destroy_process_group()


def _run(world, case, wire, steps):
    out = tempfile.mkdtemp(prefix="dl_stream_")
    ctx = mp.start_processes(_worker, args=(world, _free_port(), case, wire, steps, out),
                             nprocs=world, join=False, start_method="fork")
    deadline = time.time() + 120
    while not ctx.join(timeout=5):  # raises when a rank failed, and ends the others
        if time.time() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the gloo ranks did not finish within 120 s")
    return [dict(np.load(os.path.join(out, f"r{r}.npz"))) for r in range(world)]


def _simulate(world, case, wire, steps):
    """The simulator's state per rank after every call and after the flush."""
    H, P, tau, alpha = case
    sim = sr.StreamSim(_theta0(), world, H, P, tau, alpha, CAP, wire=wire, **HYPER)
    want = [{} for _ in range(world)]

    def snap(tag, keys):
        for r in range(world):
            for k in keys:
                want[r][f"{k}_{tag}"] = sim.flat(k, r)
    for t in range(1, steps + 1):
        sim.inner_steps()
        sim.after_inner_step()
        snap(f"t{t}", ("theta", "mom", "inner"))
    sim.flush()
    snap("end", ("theta", "mom", "inner", "wire"))
    return want


@pytest.mark.parametrize("case,wire", [((4, 2, 1, 0.5), "f32"), ((6, 3, 3, 0.3), "f32"),
                                       ((4, 2, 1, 0.5), "bf16")])
def test_two_gloo_ranks_match_the_simulator_bit_exact(case, wire):
    steps = 2 * case[0] + 1
    want = _simulate(2, case, wire, steps)
    for r, rec in enumerate(_run(2, case, wire, steps)):
        assert sorted(rec) == sorted(want[r])
        for k in want[r]:
            assert rec[k].tobytes() == want[r][k].tobytes(), (r, k)


def test_four_gloo_ranks_match_the_simulator_normwise():
    case, steps = (4, 2, 1, 0.5), 9
    numels = get_tree("micro").numels()
    want = _simulate(4, case, "f32", steps)
    recs = _run(4, case, "f32", steps)
    for r, rec in enumerate(recs):
        for k in want[r]:
            for a, b in zip(split(rec[k], numels), split(want[r][k], numels)):
                assert normwise_ok(a, b, 1e-6), (r, k)
    for k in recs[0]:  # every replica holds the same outer state
        if k.startswith(("theta", "mom")):
            assert all(rec[k].tobytes() == recs[0][k].tobytes() for rec in recs), k
