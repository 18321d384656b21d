"""Write footprints of the kernels, checked with non-zero sentinels (test helper).

The header (include/diloco_hip.h) promises that the padding of a packed buffer is never written,
that a bucket launch touches only its bucket, that inputs are only read and that results do not
depend on the tensors' alignment, the grid or the bucket split. A zero sentinel cannot pin any of
that: the SGD rule maps (g, buf, θ) = (0, 0, 0) to zeros and adam1 maps (g, m, v, θ) = (0, 0, 0,
0) to zeros (den = eps, θ = 0 + (nss·0)/eps), so a kernel that computes over and stores the
padding writes exactly the zeros such a test expects.

A Rig lays every buffer of one call out in one byte arena and builds that arena several times
from the same bytes: once for the reference (the CPU checker backends of tests/*_oracle_kernels.py,
composed into FootprintKernels) and once per grid cap for the kernels under test. Everything a
launch is not entitled to write holds a sentinel whose bits any arithmetic would change:

  packed buffers       real values in the segments, the sentinel in every padding element
  per-tensor storage   every tensor a slice of one base buffer, k elements (k = 0..3) off a 16-B
                       boundary, at least GUARD sentinel elements before and after it
  fp64 partials        a 64-bit sentinel in every entry
  q8 slots             one guard slot of sentinel bytes before and after the launch's slots, which
                       are zeroed (the padding slots of the header: zeroed once by the caller)
  flat buffers         GUARD sentinel elements before and after

After the same call on every copy the arenas are compared byte for byte, so the reference is the
statement of the values and of the footprint at once; a mismatch names the buffer, the region
(segment t / padding / guard before or after tensor t / other bucket / slot tail / header) and
the first index. tests/test_footprint_cpu.py shows that the reference itself stays inside the
footprint and that the comparison reports every kind of leak; tests/test_footprint_gpu.py runs
the rows on the GPU."""
import bisect

import numpy as np
import torch

from clip_oracle_kernels import ClipCpuTree
from diloco_amd import _lib
from diloco_amd.kernels import adamw_scalars
from diloco_amd.plan import SLOT_AUX, SLOT_GRAD, SLOT_INNER
from inner_adamw_oracle_kernels import InnerAdamWOracleKernels
from oracle import oracle
from q8_ef_oracle_kernels import Q8EFOracleKernels

F = np.float32
# the suite's ragged tree plus one tensor of exactly one chunk, which it lacks
RAGGED = [1, 3, 5, 4097, 0, 64, 65, 12345, 8191, 4096 * 3 + 7, 2, 4096]
CAP = 4096
GUARD = 64
ALL = _lib.ALL_BUCKETS
SLOT, HDR, CHUNK = oracle.Q8_SLOT, oracle.Q8_HDR, oracle.CHUNK
GRIDS = (0, 1, 2, 5)
MODES = ("whole", "buckets")
PLACES = tuple((p, p) for p in ("zero", "one", "mixed"))
PLACES2 = tuple((p, q) for p in ("zero", "one", "mixed") for q in ("zero", "one", "mixed"))

# Any arithmetic on either pattern changes its bits or the result: a signalling NaN comes back
# quiet, and the huge finite one is what fmaxf (which ignores a NaN) cannot ignore.
SENTINELS = {
    "snan": {"f32": 0x7F8BEEF5, "bf16": 0x7FA5, "f64": 0x7FF40000BEEFBEEF, "u8": 0xA5},
    "huge": {"f32": 0x7F7FBEEF, "bf16": 0x7F7E, "f64": 0x7FEFBEEFBEEFBEEF, "u8": 0x5A},
}
_UINT = {"f32": np.uint32, "bf16": np.uint16, "f64": np.uint64, "u8": np.uint8}
_TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f64": torch.float64, "u8": torch.uint8}
_SIZE = {"f32": 4, "bf16": 2, "f64": 8, "u8": 1}
ARENA_BYTES = 4 << 20
NEVER = -2  # owner of bytes no launch may write: padding, guards, gaps, inputs that have no bucket


class FootprintKernels(InnerAdamWOracleKernels, Q8EFOracleKernels):
    """Every CPU checker backend in one class (clip + inner AdamW; SGD, AdamW, shard, q8), plus
    the defer / resume pair, which has no CPU twin, restated from the header's own statement."""

    def _theta_mom(self, tree, bucket, theta, mom):
        return [(x, i, self._seg(tree, x, i).copy()) for x in (theta, mom) if x is not None
                for i in tree.segs(bucket)]

    def delta_pack_sgd_defer(self, tree, bucket, inner_slot, theta, wire, mom, lr, momentum,
                             nesterov, first):
        """The wire and inner of delta_pack_sgd; θ and the momentum keep their values."""
        kept = self._theta_mom(tree, bucket, theta, mom)
        self.delta_pack_sgd(tree, bucket, inner_slot, theta, wire, mom, lr, momentum, nesterov,
                            first)
        for x, i, v in kept:
            self._seg(tree, x, i)[:] = v

    def delta_pack_sgd_resume(self, tree, bucket, inner_slot, theta, wire, mom, pending, lr,
                              momentum, nesterov, first):
        """The pending step completed as dl_unpack_sgd(divisor 1, inner_slot -1) completes it,
        then delta_pack_sgd: with the defer before it, delta_pack_sgd twice."""
        p_lr, p_momentum, p_nesterov, p_first = pending
        self.unpack_sgd(tree, bucket, wire, 1, theta, mom, p_lr, p_momentum, p_nesterov, p_first,
                        -1)
        self.delta_pack_sgd(tree, bucket, inner_slot, theta, wire, mom, lr, momentum, nesterov,
                            first)


REF = FootprintKernels()
PLAN = ClipCpuTree(RAGGED, CAP)  # the layout, from the host-only planner
SEG_BUCKET = [b for b in range(PLAN.n_buckets) for _ in PLAN.segs(b)]
CHUNK_BUCKET = [b for b, (c0, c1) in enumerate(PLAN.bucket_chunks) for _ in range(c0, c1)]


def chunk_range(bucket):
    return (0, PLAN.n_chunks) if bucket == ALL else PLAN.bucket_chunks[bucket]


_TREES = {}


def _tree(kernels, device, grid):
    """The backend's tree of RAGGED with the walkers' grid capped at `grid` (DL_TUNE_AUTO
    flags), one per backend and cap for the whole run: a rig only rebinds its slots."""
    key = (id(kernels), str(device), grid)
    if key not in _TREES:
        tree = kernels.tree(RAGGED, torch.device(device), CAP)
        assert tree.n_chunks == PLAN.n_chunks and tree.bucket_chunks == PLAN.bucket_chunks
        assert tree.total == PLAN.total
        if hasattr(tree, "tune"):
            tree.tune(grid)
        else:
            assert grid == 0
        _TREES[key] = (tree, kernels)  # the backend stays alive, so its id stays its own
    return _TREES[key][0]


def _up(x, a):
    return -(-x // a) * a


def _bf16_bits(x):
    return (oracle.bf16_round(np.ascontiguousarray(x, F)).view(np.uint32) >> 16).astype(np.uint16)


class Buf:
    def __init__(self, name, kind, dtype, off, n, **meta):
        self.name, self.kind, self.dtype, self.off, self.n = name, kind, dtype, off, n
        self.nbytes = n * _SIZE[dtype]
        self.__dict__.update(meta)


class Feed:
    """A step that gives the real elements of a buffer new values, on every copy."""

    def __init__(self, name):
        self.name = name


class Side:
    """One copy of the arena: its tensors by buffer name, its tree and its backend."""

    def __init__(self, rig, arena, kernels, tree, label, reference=False):
        self.rig, self.arena, self.K, self.tree = rig, arena, kernels, tree
        self.label, self.reference = label, reference
        self._views = {}

    def view(self, dtype, byte_off, n):
        return self.arena[byte_off:byte_off + n * _SIZE[dtype]].view(_TORCH[dtype])

    def __getattr__(self, name):
        bufs = self.__dict__["rig"].bufs
        if name not in bufs:
            raise AttributeError(name)
        if name not in self._views:
            b = bufs[name]
            if b.kind == "slot":
                v = [self.view("f32", b.off + 4 * s, n) for s, n in zip(b.starts, RAGGED)]
            elif b.kind in ("flat", "q8flat"):
                v = self.view(b.dtype, b.off + b.body * _SIZE[b.dtype], b.len)
            else:
                v = self.view(b.dtype, b.off, b.n)
            self._views[name] = v
        return self._views[name]

    def q8(self, name, bucket):
        """The slots of a bucket's chunks: the pointer the engine passes for that launch."""
        b = self.rig.bufs[name]
        c0, c1 = chunk_range(bucket)
        return self.view("u8", b.off + SLOT * (1 + c0), SLOT * (c1 - c0))

    def dirty(self, name, bucket):
        """Garbage into the launch's own slots (bucket None: the flat slot buffer `name`) on the
        copies under test, zeros for the reference: equal bytes afterwards mean the kernel wrote
        every byte of its slots."""
        if not self.reference:
            (self.q8(name, bucket) if bucket is not None else getattr(self, name)).fill_(0xEE)


class Rig:
    def __init__(self, sentinel, place=PLACES[0], seed=2024):
        self.sent = SENTINELS[sentinel]
        self.place = place
        self.rng = np.random.default_rng(seed)
        self.init = np.full(ARENA_BYTES, self.sent["u8"], dtype=np.uint8)
        self.owner = np.full(ARENA_BYTES, NEVER, dtype=np.int16)
        self.top = 256
        self.bufs, self.order, self.binds = {}, [], []
        self.ref, self.sides = None, []

    # ---- layout ------------------------------------------------------------------------------
    def _alloc(self, name, kind, dtype, n, **meta):
        assert name not in self.bufs
        b = Buf(name, kind, dtype, self.top, n, **meta)
        self.top = _up(b.off + b.nbytes, 256) + 256  # a sentinel gap between buffers
        assert self.top <= ARENA_BYTES
        self.bufs[name] = b
        self.order.append(b)
        self._bits(b, self.init)[:] = self.sent[dtype]
        return b

    @staticmethod
    def _bits(b, arena):
        return arena[b.off:b.off + b.nbytes].view(_UINT[b.dtype])

    def _own(self, b, lo, n, bucket):
        s = _SIZE[b.dtype]
        self.owner[b.off + lo * s:b.off + (lo + n) * s] = bucket

    def _values(self, n, fill, dtype):
        x = self.rng.standard_normal(n).astype(F)
        if fill == "square":  # exp_avg_sq: never negative
            x = (x * x * F(0.01)).astype(F)
        elif fill == "small":
            x = (x * F(1e-3)).astype(F)
        elif fill == "zero":
            x = np.zeros(n, F)
        return _bf16_bits(x) if dtype == "bf16" else x.view(np.uint32)

    def _fill(self, b, arena):
        """Real (finite) values into the elements of b that hold data."""
        u = self._bits(b, arena)
        if b.kind == "packed":
            for t, n in enumerate(RAGGED):
                o = int(PLAN.seg_off[t])
                u[o:o + n] = self._values(n, b.fill, b.dtype)
        elif b.kind == "slot":
            for s, n in zip(b.starts, RAGGED):
                u[s:s + n] = self._values(n, b.fill, b.dtype)
        elif b.kind == "flat":
            u[b.body:b.body + b.len] = self._values(b.len, b.fill, b.dtype)
        else:
            raise AssertionError(b.kind)

    def packed(self, name, dtype="f32", fill="normal"):
        b = self._alloc(name, "packed", dtype, PLAN.total, fill=fill)
        for t, n in enumerate(RAGGED):
            self._own(b, int(PLAN.seg_off[t]), n, SEG_BUCKET[t])
        self._fill(b, self.init)

    def slot(self, name, slot, role=0, fill="normal"):
        """Per-tensor storage bound to `slot`: tensor t starts k_t elements past a 16-B boundary
        of one base buffer, k_t from the rig's placement for `role` (0: first bound slot)."""
        p = self.place[role]
        ks = [{"zero": 0, "one": 1}.get(p, (t + 2 + role) % 4) for t in range(len(RAGGED))]
        if p == "mixed":
            assert {2, 3} <= set(ks)
        los, starts, at = [], [], 0
        for k, n in zip(ks, RAGGED):
            los.append(at)
            starts.append(at + GUARD + k)
            at = _up(starts[-1] + n + GUARD, 4)
        los.append(at)
        b = self._alloc(name, "slot", "f32", at, fill=fill, los=los, starts=starts, slot=slot)
        for t, n in enumerate(RAGGED):
            assert (b.off + 4 * starts[t]) % 16 == 4 * ks[t]
            assert starts[t] - los[t] >= GUARD and los[t + 1] - starts[t] - n >= GUARD
            self._own(b, starts[t], n, SEG_BUCKET[t])
        self._fill(b, self.init)
        self.binds.append(b)

    def partials(self, name):
        b = self._alloc(name, "partials", "f64", PLAN.n_chunks)
        for c in range(PLAN.n_chunks):
            self._own(b, c, 1, CHUNK_BUCKET[c])

    def q8(self, name):
        b = self._alloc(name, "q8", "u8", (PLAN.n_chunks + 2) * SLOT)
        self._bits(b, self.init)[SLOT:-SLOT] = 0
        for c in range(PLAN.n_chunks):
            self._own(b, (1 + c) * SLOT, SLOT, CHUNK_BUCKET[c])

    def flat(self, name, n, dtype="f32", fill="normal", owned=True):
        """A flat buffer of n elements with guard bands; owned=False: an input, only read."""
        b = self._alloc(name, "flat", dtype, n + 2 * GUARD, fill=fill, body=GUARD, len=n)
        if owned:
            self._own(b, GUARD, n, 0)
        self._fill(b, self.init)

    def scalar(self, name, value):
        self.flat(name, 1, owned=False)
        b = self.bufs[name]
        self._bits(b, self.init)[b.body] = np.array([value], F).view(np.uint32)[0]

    def q8flat(self, name, n_slots, content=None, owned=True):
        """n_slots q8 slots (zero, or the given bytes) between two guard slots."""
        b = self._alloc(name, "q8flat", "u8", (n_slots + 2) * SLOT, body=SLOT, len=n_slots * SLOT)
        self._bits(b, self.init)[SLOT:-SLOT] = 0 if content is None else content
        if owned:
            self._own(b, SLOT, n_slots * SLOT, 0)

    # ---- the copies ---------------------------------------------------------------------------
    def commit(self, kernels=None, device="cpu", grids=(0,)):
        """The reference copy, and one copy per grid cap for `kernels` on `device`."""
        init = torch.from_numpy(self.init[:self.top])
        self.owner = self.owner[:self.top]
        self.ref = Side(self, init.clone(), REF, PLAN, "reference", reference=True)
        self.cuda = kernels is not None and torch.device(device).type == "cuda"
        for g in grids if kernels is not None else ():
            tree = _tree(kernels, device, g)
            side = Side(self, init.to(device) if self.cuda else init.clone(), kernels, tree,
                        f"grid cap {g}")
            side.grid = g
            if self.cuda:
                assert side.arena.data_ptr() % 256 == 0
            self.sides.append(side)
        for s in [self.ref] + self.sides:
            for b in self.binds:
                s.K.bind(s.tree, b.slot, getattr(s, b.name), torch.device(device))

    # ---- running ------------------------------------------------------------------------------
    def run(self, steps, mode, inside=False, empty=False):
        """Every step on every copy, whole-tree or bucket by bucket, the full comparison after
        every launch. inside: also check that the reference kept inside its footprint. empty: the
        footprint of every step is empty (otherwise the reference must have written something)."""
        buckets = [ALL] if mode == "whole" else list(range(PLAN.n_buckets))
        for s in self.sides:
            g = getattr(s, "grid", 0)
            if g and mode == "whole":
                assert g < PLAN.n_chunks  # the stride loop iterates
            if g in (1, 2) and mode == "buckets":
                assert any(g < c1 - c0 for c0, c1 in PLAN.bucket_chunks)
        wrote = False
        for k, step in enumerate(steps):
            if isinstance(step, Feed):
                self.feed(step.name)
                continue
            for b in buckets:
                before = self.ref.arena.numpy().copy()
                for s in [self.ref] + self.sides:
                    step(s.K, s.tree, s, b)
                wrote = wrote or not np.array_equal(before, self.ref.arena.numpy())
                if inside:
                    self.assert_reference_inside(before, b, f"step {k}, bucket {b}")
                self.compare(b, f"step {k}, bucket {b}")
        # equal bytes mean the kernels wrote what the reference wrote: it must have written
        if empty is not None:  # None: the step rewrites the bytes it read (an in-place copy)
            assert wrote != empty, "the reference wrote nothing" if not wrote else "not empty"

    def feed(self, name):
        b = self.bufs[name]
        self._fill(b, self.ref.arena.numpy())
        for s in self.sides:
            s.arena[b.off:b.off + b.nbytes].copy_(self.ref.arena[b.off:b.off + b.nbytes])

    def assert_reference_inside(self, before, bucket, what):
        cur = self.ref.arena.numpy()
        never = self.owner == NEVER
        bad = np.nonzero(never & (cur != self.init[:self.top]))[0]
        assert bad.size == 0, f"{what}: the reference wrote {self.where(int(bad[0]), bucket)}"
        if bucket != ALL:
            other = ~never & (self.owner != bucket)
            bad = np.nonzero(other & (cur != before))[0]
            assert bad.size == 0, f"{what}: the reference wrote {self.where(int(bad[0]), bucket)}"

    def compare(self, bucket, what):
        if self.cuda:
            torch.cuda.synchronize()
        want = self.ref.arena
        for s in self.sides:
            got = s.arena.cpu() if self.cuda else s.arena
            if torch.equal(got, want):
                continue
            bad = np.nonzero(got.numpy() != want.numpy())[0]
            first = int(bad[0])
            places = []
            for i in bad[:4096]:
                w = self.where(int(i), bucket, brief=True)
                if w not in places:
                    places.append(w)
            raise AssertionError(
                f"{what}, {s.label}: {bad.size} bytes differ from the reference; first at "
                f"{self.where(first, bucket)}: got byte 0x{int(got[first]):02x}, want "
                f"0x{int(want[first]):02x}; regions hit: {places[:8]}")

    # ---- naming a byte -----------------------------------------------------------------------
    def where(self, byte, bucket=ALL, brief=False):
        """'buffer NAME, REGION, index I' of an arena byte for a launch of `bucket`."""
        k = bisect.bisect_right([b.off for b in self.order], byte) - 1
        b = self.order[k] if k >= 0 else None
        if b is None or byte >= b.off + b.nbytes:
            return "the gap between two buffers" if brief else f"arena byte {byte}, a gap"
        i = (byte - b.off) // _SIZE[b.dtype]
        region = self._region(b, i)
        own = int(self.owner[byte])
        if bucket != ALL and own != NEVER and own != bucket:
            region = f"other bucket ({region} of bucket {own})"
        return f"buffer {b.name}, {region}" + ("" if brief else f", index {i}")

    def _region(self, b, i):
        if b.kind == "packed":
            for u in range(len(RAGGED)):
                o = int(PLAN.seg_off[u])
                if o <= i < o + RAGGED[u]:
                    return f"segment {u}"
            return "padding"
        if b.kind == "slot":
            t = bisect.bisect_right(b.los, i) - 1
            if i < b.starts[t]:
                return f"guard before tensor {t}"
            if i < b.starts[t] + RAGGED[t]:
                return f"segment {t}"
            return f"guard after tensor {t}"
        if b.kind == "partials":
            return f"partial of chunk {i}"
        if b.kind in ("q8", "q8flat"):
            j, r = divmod(i, SLOT)
            n_slots = b.n // SLOT - 2
            if j == 0:
                return "guard slot before"
            if j == n_slots + 1:
                return "guard slot after"
            part = "scale" if r < 4 else "header" if r < HDR else "payload"
            if b.kind == "q8" and r >= HDR + PLAN.chunks[j - 1][2]:
                part = "slot tail"
            return f"{part} of slot {j - 1}"
        if i < b.body:
            return "guard before"
        return "body" if i < b.body + b.len else "guard after"


class Case:
    def __init__(self, name, setup, steps, places=PLACES, empty=False):
        self.name, self.setup, self.steps, self.places = name, setup, steps, places
        self.empty = empty  # no step may write anything


def run_case(case, kernels=None, device="cpu", grids=(0,), sentinels=tuple(SENTINELS),
             modes=MODES, places=None):
    """One row: every sentinel, placement and launch mode, all grid caps side by side.
    kernels None: the reference alone, checked against its own footprint."""
    for sentinel in sentinels:
        for place in places or case.places:
            for mode in modes:
                rig = Rig(sentinel, place)
                case.setup(rig)
                if not rig.binds and place != (places or case.places)[0]:
                    continue  # no per-tensor storage: nothing to place differently
                rig.commit(kernels, device, grids)
                try:
                    rig.run(case.steps, mode, inside=kernels is None, empty=case.empty)
                except AssertionError as e:
                    raise AssertionError(f"{case.name} [{sentinel} sentinel, placement {place}, "
                                         f"{mode}]: {e}") from None


def run_flat_case(case, kernels=None, device="cpu"):
    """A flat-kernel row: no tree, one launch per step, one copy under test."""
    run_case(case, kernels, device, modes=("whole",), places=PLACES[:1])


# ---- the rows: tree walkers ------------------------------------------------------------------
LR, MOMENTUM = 0.7, 0.9
ADAM = [adamw_scalars(0.01, 0.9, 0.95, 0.1, 1e-8, t) for t in (1, 2)]
WIRES = ("f32", "bf16")


def _buffers(*specs):
    """setup(rig) from (maker, name, ...) tuples."""
    def setup(rig):
        for maker, *args in specs:
            kw = args.pop() if args and isinstance(args[-1], dict) else {}
            getattr(rig, maker)(*args, **kw)
    return setup


def _sgd_state(wire=None, inner=True, mom=True):
    specs = [("packed", "theta")]
    if mom:
        specs.append(("packed", "mom", {"fill": "small"}))
    if wire:
        specs.append(("packed", "wire", wire))
    if inner:
        specs.append(("slot", "inner", SLOT_INNER))
    return specs


def _adam_state(wire=None, inner=True):
    specs = [("packed", "theta"), ("packed", "m", {"fill": "small"}),
             ("packed", "v", {"fill": "square"})]
    if wire:
        specs.append(("packed", "wire", wire))
    if inner:
        specs.append(("slot", "inner", SLOT_INNER))
    return specs


def _sgd_modes():
    """(label, momentum, nesterov): momentum 0, and a momentum with and without Nesterov; the two
    consecutive calls of a case are the first-step mode and then the steady one."""
    return [("momentum 0", 0.0, False), ("nesterov", MOMENTUM, True), ("plain", MOMENTUM, False)]


def cases_delta_pack(wire):
    call = lambda K, T, S, b: K.delta_pack(T, b, SLOT_INNER, S.theta, S.wire)  # noqa: E731
    yield Case(f"delta_pack {wire}", _buffers(*_sgd_state(wire, mom=False)),
               [call, Feed("inner"), call])


def cases_gather(dtype):
    call = lambda K, T, S, b: K.gather(T, b, SLOT_GRAD, S.packed)  # noqa: E731
    yield Case(f"gather {dtype}", _buffers(("slot", "grads", SLOT_GRAD), ("packed", "packed", dtype)),
               [call, Feed("grads"), call])


def cases_scatter():
    call = lambda K, T, S, b: K.scatter(T, b, S.theta, SLOT_INNER)  # noqa: E731
    yield Case("scatter", _buffers(*_sgd_state(mom=False)), [call, Feed("theta"), call])


def _unpack_avg_cases(wire, sumsq):
    name = "unpack_avg_sumsq" if sumsq else "unpack_avg"
    dests = ("slot", "packed") + (("in place",) if wire == "f32" else ())
    for dest in dests:
        for divisor in (1, 3):
            specs = [("packed", "wire", wire)]
            if dest == "slot":
                specs.append(("slot", "grads", SLOT_GRAD))
            if dest == "packed":
                specs.append(("packed", "dst"))
            if sumsq:
                specs.append(("partials", "partials"))

            def call(K, T, S, b, dest=dest, divisor=divisor):
                slot = SLOT_GRAD if dest == "slot" else -1
                dst = None if dest == "slot" else S.dst if dest == "packed" else S.wire
                if sumsq:
                    K.unpack_avg_sumsq(T, b, S.wire, divisor, slot, S.partials, dst)
                else:
                    K.unpack_avg(T, b, S.wire, divisor, slot, dst)
            yield Case(f"{name} {wire} to {dest}, divisor {divisor}", _buffers(*specs),
                       [call, Feed("wire"), call],
                       empty=None if dest == "in place" and divisor == 1 and not sumsq else False)


def cases_unpack_avg(wire):
    return _unpack_avg_cases(wire, False)


def cases_unpack_avg_sumsq(wire):
    return _unpack_avg_cases(wire, True)


def cases_grad_sumsq():
    call = lambda K, T, S, b: K.grad_sumsq(T, b, SLOT_GRAD, S.partials)  # noqa: E731
    yield Case("grad_sumsq", _buffers(("slot", "grads", SLOT_GRAD), ("partials", "partials")),
               [call, Feed("grads"), call])


def cases_scale_by():
    for coef in (0.37, 1.0):  # 1.0: the footprint is empty
        call = lambda K, T, S, b: K.scale_by(T, b, SLOT_GRAD, S.coef)  # noqa: E731
        yield Case(f"scale_by {coef}", _buffers(("slot", "grads", SLOT_GRAD),
                                                 ("scalar", "coef", coef)), [call, call],
                   empty=coef == 1.0)


def cases_unpack_sgd(wire):
    for label, momentum, nesterov in _sgd_modes():
        for inner in (True, False):
            def call(first, momentum=momentum, nesterov=nesterov, inner=inner):
                return lambda K, T, S, b: K.unpack_sgd(
                    T, b, S.wire, 3, S.theta, S.mom if momentum else None, LR, momentum, nesterov,
                    first, SLOT_INNER if inner else -1)
            yield Case(f"unpack_sgd {wire}, {label}, inner {inner}",
                       _buffers(*_sgd_state(wire, inner, bool(momentum))),
                       [call(True), Feed("wire"), call(False)])


def cases_delta_sgd():
    for label, momentum, nesterov in _sgd_modes():
        def call(first, momentum=momentum, nesterov=nesterov):
            return lambda K, T, S, b: K.delta_sgd(T, b, SLOT_INNER, S.theta,
                                                  S.mom if momentum else None, LR, momentum,
                                                  nesterov, first)
        yield Case(f"delta_sgd, {label}", _buffers(*_sgd_state(None, True, bool(momentum))),
                   [call(True), Feed("inner"), call(False)])


def cases_delta_pack_sgd(wire):
    for label, momentum, nesterov in _sgd_modes():
        def call(first, momentum=momentum, nesterov=nesterov):
            return lambda K, T, S, b: K.delta_pack_sgd(T, b, SLOT_INNER, S.theta, S.wire,
                                                       S.mom if momentum else None, LR, momentum,
                                                       nesterov, first)
        yield Case(f"delta_pack_sgd {wire}, {label}",
                   _buffers(*_sgd_state(wire, True, bool(momentum))),
                   [call(True), Feed("inner"), call(False)])


def cases_defer_resume():
    """defer (the first step), resume (the steady one), then a second defer / resume pair whose
    pending step is a steady one."""
    for label, momentum, nesterov in _sgd_modes():
        def defer(first, momentum=momentum, nesterov=nesterov):
            return lambda K, T, S, b: K.delta_pack_sgd_defer(
                T, b, SLOT_INNER, S.theta, S.wire, S.mom if momentum else None, LR, momentum,
                nesterov, first)

        def resume(p_first, momentum=momentum, nesterov=nesterov):
            return lambda K, T, S, b: K.delta_pack_sgd_resume(
                T, b, SLOT_INNER, S.theta, S.wire, S.mom if momentum else None,
                (LR, momentum, nesterov, p_first), 0.5, momentum, nesterov, False)
        yield Case(f"delta_pack_sgd_defer / resume, {label}",
                   _buffers(*_sgd_state("f32", True, bool(momentum))),
                   [defer(True), Feed("inner"), resume(True), Feed("inner"), defer(False),
                    Feed("inner"), resume(False)])


def cases_pack_sgd_tiled(wire):
    for tile in (1, 3):
        def call(first, tile=tile):
            return lambda K, T, S, b: K.pack_sgd_tiled(T, b, SLOT_INNER, S.theta, S.wire, S.mom, LR,
                                                       MOMENTUM, True, first, tile)
        yield Case(f"pack_sgd_tiled {wire}, tile_chunks {tile}", _buffers(*_sgd_state(wire)),
                   [call(True), Feed("inner"), call(False)])


def cases_unpack_adamw(wire):
    for divisor in (1, 3):
        for inner in (True, False):
            def call(t, divisor=divisor, inner=inner):
                return lambda K, T, S, b: K.unpack_adamw(T, b, S.wire, divisor, S.theta, S.m, S.v,
                                                         ADAM[t], SLOT_INNER if inner else -1)
            yield Case(f"unpack_adamw {wire}, divisor {divisor}, inner {inner}",
                       _buffers(*_adam_state(wire, inner)), [call(0), Feed("wire"), call(1)])


def cases_delta_pack_adamw(wire):
    def call(t):
        return lambda K, T, S, b: K.delta_pack_adamw(T, b, SLOT_INNER, S.theta, S.wire, S.m, S.v,
                                                     ADAM[t])
    yield Case(f"delta_pack_adamw {wire}", _buffers(*_adam_state(wire)),
               [call(0), Feed("inner"), call(1)])


def cases_adamw_step():
    """params and grads are placed independently: every pair of placements."""
    for coef in (None, 0.37):
        specs = [("slot", "params", SLOT_INNER), ("slot", "grads", SLOT_GRAD, 1),
                 ("packed", "m", {"fill": "small"}), ("packed", "v", {"fill": "square"})]
        if coef is not None:
            specs.append(("scalar", "coef", coef))

        def call(t, coef=coef):
            return lambda K, T, S, b: K.adamw_step(T, b, SLOT_INNER, SLOT_GRAD, S.m, S.v, ADAM[t],
                                                   None if coef is None else S.coef)
        yield Case(f"adamw_step, coef {coef}", _buffers(*specs), [call(0), Feed("grads"), call(1)],
                   places=PLACES2)


def _encode(ef, dirty=False):
    def call(K, T, S, b):
        if dirty:
            S.dirty("slots", b)
        if ef:
            K.delta_q8_ef(T, b, SLOT_INNER, S.theta, S.resid, S.q8("slots", b))
        else:
            K.delta_q8(T, b, SLOT_INNER, S.theta, S.q8("slots", b))
    return call


def cases_delta_q8(ef=False):
    """dirty: the encoder owns every byte of its slots (the header, and zeros past the chunk's
    length), so garbage there beforehand must not survive."""
    name = "delta_q8_ef" if ef else "delta_q8"
    specs = _sgd_state(mom=False) + [("q8", "slots")]
    if ef:
        specs.append(("packed", "resid", {"fill": "small"}))
    for dirty in (False, True):
        yield Case(f"{name}{', dirty slots' if dirty else ''}", _buffers(*specs),
                   [_encode(ef, dirty), Feed("inner"), _encode(ef, dirty)])


def cases_delta_q8_ef():
    return cases_delta_q8(ef=True)


def cases_unpack_sgd_q8():
    """The slots come from dl_delta_q8 on the same rig, so both copies decode equal bytes."""
    for label, momentum, nesterov in _sgd_modes():
        for inner in (True, False):
            def call(first, momentum=momentum, nesterov=nesterov, inner=inner):
                return lambda K, T, S, b: K.unpack_sgd_q8(
                    T, b, S.q8("slots", b), S.theta, S.mom if momentum else None, LR, momentum,
                    nesterov, first, SLOT_INNER if inner else -1)
            specs = _sgd_state(None, inner, bool(momentum)) + [("slot", "peer", SLOT_AUX, 1),
                                                               ("q8", "slots")]
            enc = lambda K, T, S, b: K.delta_q8(T, b, SLOT_AUX, S.theta, S.q8("slots", b))  # noqa: E731
            yield Case(f"unpack_sgd_q8, {label}, inner {inner}", _buffers(*specs),
                       [enc, call(True), Feed("peer"), enc, call(False)])


def cases_unpack_adamw_q8():
    for inner in (True, False):
        def call(t, inner=inner):
            return lambda K, T, S, b: K.unpack_adamw_q8(T, b, S.q8("slots", b), S.theta, S.m, S.v,
                                                        ADAM[t], SLOT_INNER if inner else -1)
        specs = _adam_state(None, inner) + [("slot", "peer", SLOT_AUX, 1), ("q8", "slots")]
        enc = lambda K, T, S, b: K.delta_q8(T, b, SLOT_AUX, S.theta, S.q8("slots", b))  # noqa: E731
        yield Case(f"unpack_adamw_q8, inner {inner}", _buffers(*specs),
                   [enc, call(0), Feed("peer"), enc, call(1)])


TREE_ROWS = {
    "delta_pack": (cases_delta_pack, WIRES), "gather": (cases_gather, WIRES),
    "scatter": (cases_scatter, None), "unpack_avg": (cases_unpack_avg, WIRES),
    "unpack_avg_sumsq": (cases_unpack_avg_sumsq, WIRES), "grad_sumsq": (cases_grad_sumsq, None),
    "scale_by": (cases_scale_by, None), "unpack_sgd": (cases_unpack_sgd, WIRES),
    "delta_sgd": (cases_delta_sgd, None), "delta_pack_sgd": (cases_delta_pack_sgd, WIRES),
    "delta_pack_sgd_defer_resume": (cases_defer_resume, None),
    "pack_sgd_tiled": (cases_pack_sgd_tiled, WIRES), "unpack_adamw": (cases_unpack_adamw, WIRES),
    "delta_pack_adamw": (cases_delta_pack_adamw, WIRES), "adamw_step": (cases_adamw_step, None),
    "delta_q8": (cases_delta_q8, None), "delta_q8_ef": (cases_delta_q8_ef, None),
    "unpack_sgd_q8": (cases_unpack_sgd_q8, None), "unpack_adamw_q8": (cases_unpack_adamw_q8, None),
}


# ---- the rows: flat kernels (no tree; bucket ALL, one copy under test) ------------------------
SHARD_N = (1, 3, 4096, 4097, 3 * 4096 + 7)
SLICE_LEN = (4, 4096, 4100, 3 * 4096 + 8)
N_SLICES = (1, 2, 3, 9)  # below and above the unrolled slice loops


def cases_shard_sgd():
    for n in SHARD_N:
        for divisor in (1, 3):
            def call(first, divisor=divisor):
                return lambda K, T, S, b: K.shard_sgd(S.wire, divisor, S.theta, S.mom, LR, MOMENTUM,
                                                      True, first)
            yield Case(f"shard_sgd n {n}, divisor {divisor}",
                       _buffers(("flat", "wire", n, {"owned": False}), ("flat", "theta", n),
                                ("flat", "mom", n, {"fill": "small"})), [call(True), call(False)])


def cases_shard_adamw():
    for n in SHARD_N:
        for wire in WIRES:
            def call(t):
                return lambda K, T, S, b: K.shard_adamw(S.wire, 3, S.theta, S.m, S.v, ADAM[t])
            yield Case(f"shard_adamw n {n}, {wire}",
                       _buffers(("flat", "wire", n, wire, {"owned": False}), ("flat", "theta", n),
                                ("flat", "m", n, {"fill": "small"}),
                                ("flat", "v", n, {"fill": "square"})), [call(0), call(1)])


def _slice_cases(name, state, call):
    for n in SLICE_LEN:
        for q in N_SLICES:
            yield Case(f"{name} len {n}, {q} slices",
                       _buffers(("flat", "slices", q * n, {"owned": False}), *state(n)),
                       [call(q, 0), call(q, 1)])


def cases_shard_reduce_sgd():
    return _slice_cases(
        "shard_reduce_sgd",
        lambda n: [("flat", "theta", n), ("flat", "mom", n, {"fill": "small"})],
        lambda q, t: lambda K, T, S, b: K.shard_reduce_sgd(S.slices, q, S.theta, S.mom, LR, MOMENTUM,
                                                           True, t == 0))


def cases_shard_reduce_avg():
    return _slice_cases("shard_reduce_avg", lambda n: [("flat", "out", n)],
                        lambda q, t: lambda K, T, S, b: K.shard_reduce_avg(S.slices, q, S.out))


def cases_shard_reduce_adamw():
    for avg in (False, True):
        def state(n, avg=avg):
            return [("flat", "theta", n), ("flat", "m", n, {"fill": "small"}),
                    ("flat", "v", n, {"fill": "square"})] + ([("flat", "avg", n)] if avg else [])

        def call(q, t, avg=avg):
            return lambda K, T, S, b: K.shard_reduce_adamw(S.slices, q, S.theta, S.m, S.v, ADAM[t],
                                                           S.avg if avg else None)
        yield from _slice_cases(f"shard_reduce_adamw{' with avg_out' if avg else ''}", state, call)


def _recv_slots(n_peers, seed=7):
    """n_peers x 3 slots: a full chunk, a short one (zero tail) and an all-zero padding slot."""
    rng = np.random.default_rng(seed)
    recv = np.zeros(n_peers * 3 * SLOT, dtype=np.uint8)
    for r in range(n_peers):
        for j, n in enumerate((CHUNK, 1000)):
            x = (1e-3 * rng.standard_normal(n)).astype(F)
            x[rng.integers(n)] = 1.0 + r
            at = (r * 3 + j) * SLOT
            recv[at:at + SLOT] = oracle.delta_q8_from(x)
    return recv


def cases_q8_reduce(ef=False):
    """n_peers 1 in place (out is recv), n_peers 2 into guarded output slots; divisor = n_peers.
    With error feedback the residual is non-zero where the slots hold values."""
    for n_peers, dirty in ((1, False), (2, False), (2, True)):
        def setup(rig, n_peers=n_peers):
            rig.q8flat("recv", n_peers * 3, _recv_slots(n_peers), owned=n_peers == 1)
            if n_peers > 1:
                rig.q8flat("out", 3)
            if ef:
                rig.flat("resid", 3 * CHUNK, fill="zero")
                b = rig.bufs["resid"]
                rig._bits(b, rig.init)[b.body:b.body + CHUNK + 1000] = rig._values(
                    CHUNK + 1000, "small", "f32")

        def call(K, T, S, b, n_peers=n_peers, dirty=dirty):
            out = S.recv if n_peers == 1 else S.out
            if dirty:  # the reduce owns every byte of its output slots
                S.dirty("out", None)
            if ef:
                K.q8_reduce_ef(S.recv, n_peers, 3, n_peers, S.resid, out)
            else:
                K.q8_reduce(S.recv, n_peers, 3, n_peers, out)
        yield Case(f"q8_reduce{'_ef' if ef else ''}, {n_peers} peers"
                   f"{', dirty output slots' if dirty else ''}", setup, [call, call],
                   empty=None if n_peers == 1 and not ef else False)  # own slots re-quantise exactly


def cases_q8_reduce_ef():
    return cases_q8_reduce(ef=True)


FLAT_ROWS = {
    "shard_sgd": cases_shard_sgd, "shard_adamw": cases_shard_adamw,
    "shard_reduce_sgd": cases_shard_reduce_sgd, "shard_reduce_avg": cases_shard_reduce_avg,
    "shard_reduce_adamw": cases_shard_reduce_adamw, "q8_reduce": cases_q8_reduce,
    "q8_reduce_ef": cases_q8_reduce_ef,
}
