"""The footprint checks' own ground, without a GPU (tests/footprint.py).

The GPU comparison means something only if (a) the CPU checker backends themselves never write a
planted sentinel nor, in a single-bucket call, anything of another bucket, (b) the byte comparison
reports every kind of leak under the right region name, and (c) the tree has the shapes at which
walkers go wrong. The leaks come from a deliberately leaky host-side subclass of the checker
backend: host tensors only, no device code is altered."""
import pytest
import torch

import footprint as fp
from footprint import ALL, CHUNK, HDR, PLAN, RAGGED, SLOT
from diloco_amd.plan import SLOT_INNER


def test_the_tree_has_the_shapes_walkers_go_wrong_at():
    assert PLAN.n_buckets >= 3
    assert 0 in RAGGED
    assert any(0 < n < 4 for n in RAGGED)
    assert {1, 2, 3} <= {n % 4 for n in RAGGED}
    assert any(n > 0 and n % CHUNK == 0 for n in RAGGED)
    assert any(n % CHUNK for n in RAGGED if n > CHUNK)  # a last chunk shorter than 4096
    assert any(c1 - c0 >= 4 for c0, c1 in PLAN.bucket_chunks)
    assert PLAN.n_chunks == 19 and len(PLAN.chunks) == 19
    for b, (lo, hi) in enumerate(PLAN.bucket_ranges):
        used = sum(RAGGED[i] for i in PLAN.segs(b))
        assert hi - lo > used or b == PLAN.n_buckets - 1, b  # non-empty padding
    rig = fp.Rig("snan", fp.PLACES[2])
    rig.slot("inner", SLOT_INNER)
    rig.packed("theta")
    assert (rig.owner[:rig.top] == fp.NEVER).sum() > 4 * fp.GUARD * len(RAGGED)


def test_the_sentinels_are_what_they_claim():
    import numpy as np

    s, h = fp.SENTINELS["snan"], fp.SENTINELS["huge"]
    f32 = np.array([s["f32"], h["f32"]], np.uint32).view(np.float32)
    assert np.isnan(f32[0]) and not s["f32"] & 0x00400000  # signalling: the quiet bit is clear
    assert np.isfinite(f32[1]) and f32[1] > 3e38
    bf = (np.array([s["bf16"], h["bf16"]], np.uint32) << 16).view(np.float32)
    assert np.isnan(bf[0]) and not s["bf16"] & 0x0040 and np.isfinite(bf[1]) and bf[1] > 3e38
    f64 = np.array([s["f64"], h["f64"]], np.uint64).view(np.float64)
    assert np.isnan(f64[0]) and not s["f64"] & (1 << 51) and np.isfinite(f64[1])
    with np.errstate(all="ignore"):  # arithmetic changes the bits
        assert (f32[:1] + np.float32(0.0)).view(np.uint32)[0] != s["f32"]  # comes back quiet
        assert (f32[1:] * np.float32(0.999)).view(np.uint32)[0] != h["f32"]


def _tree_cases():
    for name, (cases, wires) in fp.TREE_ROWS.items():
        for w in wires or (None,):
            yield pytest.param(cases, w, id=name + (f"-{w}" if w else ""))


@pytest.mark.parametrize("cases, wire", _tree_cases())
def test_the_reference_stays_inside_the_footprint(cases, wire):
    """Every tree-walker row, both sentinels, whole-tree and bucket by bucket: after the CPU
    backend's call every planted sentinel is still there, and a single-bucket call leaves every
    other bucket's segments, slots and partials bit-identical. One placement: the host backend
    has no alignment paths."""
    for case in cases(wire) if wire else cases():
        if "dirty" in case.name:
            continue  # a statement about the kernel's slots; the reference's are zeroed
        fp.run_case(case, places=fp.PLACES[2:])


@pytest.mark.parametrize("row", list(fp.FLAT_ROWS))
def test_the_flat_reference_stays_inside_the_footprint(row):
    for case in fp.FLAT_ROWS[row]():
        fp.run_flat_case(case)


def _leaky(method, poke):
    """The checker backend with `poke(tree, bucket, *args)` run after `method`."""
    class Leaky(fp.FootprintKernels):
        pass

    def wrapped(self, tree, bucket, *args, **kw):
        getattr(fp.FootprintKernels, method)(self, tree, bucket, *args, **kw)
        poke(tree, bucket, *args, **kw)
    setattr(Leaky, method, wrapped)
    return Leaky()


def _first(gen):
    return next(iter(gen))


def _expect(case, method, poke, region, modes=fp.MODES):
    fp.run_case(case, fp.FootprintKernels(), "cpu", modes=modes, places=fp.PLACES[2:])  # clean
    with pytest.raises(AssertionError, match=region):
        fp.run_case(case, _leaky(method, poke), "cpu", modes=modes, places=fp.PLACES[2:])


def _past(t, k):
    """Element k of tensor t's storage, counted from its start (k < 0: before it)."""
    return torch.as_strided(t, (1,), (1,), t.storage_offset() + k)


def test_a_zero_in_the_padding_is_reported():
    def poke(tree, bucket, inner_slot, theta, wire):
        wire[int(tree.seg_off[0]) + RAGGED[0]] = 0
    _expect(_first(fp.cases_delta_pack("f32")), "delta_pack", poke, "buffer wire, padding")
    _expect(_first(fp.cases_delta_pack("bf16")), "delta_pack", poke, "buffer wire, padding")


def test_a_store_past_a_tensors_end_and_before_its_start_are_reported():
    def past(tree, bucket, packed, dst_slot):
        t = tree.slots[dst_slot][3]
        if bucket in (ALL, fp.SEG_BUCKET[3]):
            _past(t, t.numel())[0] = 1.0

    def before(tree, bucket, packed, dst_slot):
        t = tree.slots[dst_slot][7]
        if bucket in (ALL, fp.SEG_BUCKET[7]):
            _past(t, -1)[0] = 1.0
    _expect(_first(fp.cases_scatter()), "scatter", past, "buffer inner, guard after tensor 3")
    _expect(_first(fp.cases_scatter()), "scatter", before, "buffer inner, guard before tensor 7")


def test_a_write_into_another_buckets_segment_is_reported():
    def poke(tree, bucket, wire, divisor, theta, *rest):
        nxt = int(tree.bounds[(bucket + 1) % tree.n_buckets])  # its first segment
        o = int(tree.seg_off[nxt])
        theta[o] = theta[o] + 1.0
    _expect(_first(fp.cases_unpack_sgd("f32")), "unpack_sgd", poke,
            "buffer theta, other bucket", modes=("buckets",))


def test_an_input_changed_in_place_is_reported():
    def poke(tree, bucket, inner_slot, theta, wire):
        theta[0] = theta[0] * 2.0
    _expect(_first(fp.cases_delta_pack("f32")), "delta_pack", poke, "buffer theta, segment 0")

    def grads(tree, bucket, src_slot, partials):
        tree.slots[src_slot][1][2] += 1.0
    _expect(_first(fp.cases_grad_sumsq()), "grad_sumsq", grads, "buffer grads, segment 1")


def test_a_slot_byte_past_the_chunks_length_is_reported():
    def poke(tree, bucket, inner_slot, theta, slots):
        c0, _ = fp.chunk_range(bucket)
        c = 0 if bucket == ALL else c0
        slots[(c - c0) * SLOT + HDR + PLAN.chunks[c][2]] = 1
    _expect(_first(fp.cases_delta_q8()), "delta_q8", poke, "buffer slots, slot tail of slot 0")

    def header(tree, bucket, inner_slot, theta, slots):
        slots[5] = 1
    _expect(_first(fp.cases_delta_q8()), "delta_q8", header, "buffer slots, header of slot")

    def guard(tree, bucket, inner_slot, theta, slots):
        _past(slots, slots.numel())[0] = 1
    _expect(_first(fp.cases_delta_q8()), "delta_q8", guard,
            "buffer slots, (guard slot after|other bucket)")


def test_a_partial_outside_the_buckets_chunk_range_is_reported():
    def poke(tree, bucket, src_slot, partials):
        _, c1 = fp.chunk_range(bucket)
        partials[c1 % PLAN.n_chunks] = 0.0
    _expect(_first(fp.cases_grad_sumsq()), "grad_sumsq", poke,
            "buffer partials, other bucket \\(partial of chunk", modes=("buckets",))


def test_a_flat_kernels_guard_bands_are_watched():
    def poke(wire, divisor, theta, *rest):
        _past(theta, theta.numel())[0] = 0.0
    case = _first(fp.cases_shard_sgd())
    fp.run_flat_case(case, fp.FootprintKernels(), "cpu")
    leaky = fp.FootprintKernels()
    clean = leaky.shard_sgd
    leaky.shard_sgd = lambda *a: (clean(*a), poke(*a))
    with pytest.raises(AssertionError, match="buffer theta, guard after"):
        fp.run_flat_case(case, leaky, "cpu")
