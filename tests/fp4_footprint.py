"""Write-footprint rows of the four fp4-wire kernels, on the helpers of tests/footprint.py.
TEST HELPER.

footprint.Rig lays the buffers of a call out in one byte arena of sentinels and compares every
byte with the CPU reference after every launch. Here the arena gains fp4 slot buffers
(DL_FP4_SLOT_BYTES slots between two guard slots of sentinel bytes, the launch's own slots
zeroed as the caller zeroes padding slots) and the reference gains the fp4 stand-ins
(tests/fp4_oracle_kernels.py). `dirty` fills the launch's slots with garbage on the copies under
test only: equal bytes afterwards mean every byte of every launched slot was written."""
import numpy as np

import footprint as fpt
import fp4_restatement as fp4
from diloco_amd.plan import SLOT_AUX, SLOT_INNER
from fp4_oracle_kernels import Fp4OracleKernels

S4, CHUNK = fp4.SLOT, fp4.CHUNK
PLAN, ALL = fpt.PLAN, fpt.ALL


class Fp4FootprintKernels(fpt.FootprintKernels, Fp4OracleKernels):
    pass


REF = Fp4FootprintKernels()


class Rig(fpt.Rig):
    def fp4(self, name):
        """One slot per chunk of the tree, a guard slot before and after."""
        b = self._alloc(name, "flat", "u8", (PLAN.n_chunks + 2) * S4, body=S4,
                        len=PLAN.n_chunks * S4)
        self._bits(b, self.init)[S4:-S4] = 0
        for c in range(PLAN.n_chunks):
            self._own(b, (1 + c) * S4, S4, fpt.CHUNK_BUCKET[c])

    def fp4flat(self, name, n_slots, content=None, owned=True):
        """n_slots slots (zero, or the given bytes) between two guard slots."""
        b = self._alloc(name, "flat", "u8", (n_slots + 2) * S4, body=S4, len=n_slots * S4)
        self._bits(b, self.init)[S4:-S4] = 0 if content is None else content
        if owned:
            self._own(b, S4, n_slots * S4, 0)

    def commit(self, kernels=None, device="cpu", grids=(0,)):
        super().commit(kernels, device, grids)
        self.ref.K = REF  # the same tree and bindings, the backend that knows the fp4 calls


def slots_of(S, name, bucket):
    """The slots of a bucket's chunks: the pointer the mirror passes for that launch."""
    b = S.rig.bufs[name]
    c0, c1 = fpt.chunk_range(bucket)
    return S.view("u8", b.off + S4 * (1 + c0), S4 * (c1 - c0))


def _dirty(S, t):
    if not S.reference:
        t.fill_(0xEE)


def run_case(case, kernels=None, device="cpu", grids=(0,), modes=fpt.MODES, places=None):
    """footprint.run_case on the Rig above."""
    for sentinel in fpt.SENTINELS:
        for place in places or case.places:
            for mode in modes:
                rig = Rig(sentinel, place)
                case.setup(rig)
                if not rig.binds and place != (places or case.places)[0]:
                    continue
                rig.commit(kernels, device, grids)
                try:
                    rig.run(case.steps, mode, inside=kernels is None, empty=case.empty)
                except AssertionError as e:
                    raise AssertionError(f"{case.name} [{sentinel} sentinel, placement {place}, "
                                         f"{mode}]: {e}") from None


def _encode(ef, dirty=False, slot=SLOT_INNER):
    def call(K, T, S, b):
        if dirty:
            _dirty(S, slots_of(S, "slots", b))
        K.delta_fp4(T, b, slot, S.theta, S.resid if ef else None, slots_of(S, "slots", b))
    return call


def cases_delta_fp4(ef):
    specs = fpt._sgd_state(mom=False) + [("fp4", "slots")]
    if ef:
        specs.append(("packed", "resid", {"fill": "small"}))
    for dirty in (False, True):
        yield fpt.Case(f"delta_fp4{' with residual' if ef else ''}{', dirty slots' if dirty else ''}",
                       fpt._buffers(*specs), [_encode(ef, dirty), fpt.Feed("inner"),
                                              _encode(ef, dirty)])


def cases_unpack_sgd_fp4():
    """The slots come from dl_delta_fp4 on the same rig, so both copies decode equal bytes."""
    for label, momentum, nesterov in fpt._sgd_modes():
        for inner in (True, False):
            def call(first, momentum=momentum, nesterov=nesterov, inner=inner):
                return lambda K, T, S, b: K.unpack_sgd_fp4(
                    T, b, slots_of(S, "slots", b), S.theta, S.mom if momentum else None, fpt.LR,
                    momentum, nesterov, first, SLOT_INNER if inner else -1)
            specs = fpt._sgd_state(None, inner, bool(momentum)) + [("slot", "peer", SLOT_AUX, 1),
                                                                   ("fp4", "slots")]
            enc = _encode(False, slot=SLOT_AUX)
            yield fpt.Case(f"unpack_sgd_fp4, {label}, inner {inner}", fpt._buffers(*specs),
                           [enc, call(True), fpt.Feed("peer"), enc, call(False)])


def cases_unpack_adamw_fp4():
    for inner in (True, False):
        def call(t, inner=inner):
            return lambda K, T, S, b: K.unpack_adamw_fp4(
                T, b, slots_of(S, "slots", b), S.theta, S.m, S.v, fpt.ADAM[t],
                SLOT_INNER if inner else -1)
        specs = fpt._adam_state(None, inner) + [("slot", "peer", SLOT_AUX, 1), ("fp4", "slots")]
        enc = _encode(False, slot=SLOT_AUX)
        yield fpt.Case(f"unpack_adamw_fp4, inner {inner}", fpt._buffers(*specs),
                       [enc, call(0), fpt.Feed("peer"), enc, call(1)])


def recv_slots(n_peers, seed=7):
    """n_peers x 3 slots: a full chunk, a short one (zero tail) and an all-zero padding slot."""
    rng = np.random.default_rng(seed)
    recv = np.zeros(n_peers * 3 * S4, dtype=np.uint8)
    for r in range(n_peers):
        for j, n in enumerate((CHUNK, 1000)):
            x = (1e-3 * rng.standard_normal(n)).astype(np.float32)
            x[rng.integers(n)] = 1.0 + r
            at = (r * 3 + j) * S4
            recv[at:at + S4] = fp4.encode_values(x)
    return recv


def cases_fp4_reduce(ef):
    """n_peers 1 in place (out is recv), n_peers 2 into guarded output slots; divisor = n_peers.
    With error feedback the residual is non-zero where the slots hold values."""
    for n_peers, dirty in ((1, False), (2, False), (2, True)):
        def setup(rig, n_peers=n_peers):
            rig.fp4flat("recv", n_peers * 3, recv_slots(n_peers), owned=n_peers == 1)
            if n_peers > 1:
                rig.fp4flat("out", 3)
            if ef:
                rig.flat("resid", 3 * CHUNK, fill="zero")
                b = rig.bufs["resid"]
                rig._bits(b, rig.init)[b.body:b.body + CHUNK + 1000] = rig._values(
                    CHUNK + 1000, "small", "f32")

        def call(K, T, S, b, n_peers=n_peers, dirty=dirty):
            out = S.recv if n_peers == 1 else S.out
            if dirty:  # the reduce owns every byte of its output slots
                _dirty(S, S.out)
            K.fp4_reduce(S.recv, n_peers, 3, n_peers, S.resid if ef else None, out)
        yield fpt.Case(f"fp4_reduce{' with residual' if ef else ''}, {n_peers} peers"
                       f"{', dirty output slots' if dirty else ''}", setup, [call, call],
                       empty=None if n_peers == 1 and not ef else False)  # decoded values re-encode


TREE_ROWS = {
    "delta_fp4": lambda: cases_delta_fp4(False), "delta_fp4_ef": lambda: cases_delta_fp4(True),
    "unpack_sgd_fp4": cases_unpack_sgd_fp4, "unpack_adamw_fp4": cases_unpack_adamw_fp4,
}
FLAT_ROWS = {"fp4_reduce": lambda: cases_fp4_reduce(False),
             "fp4_reduce_ef": lambda: cases_fp4_reduce(True)}


def run_flat_case(case, kernels=None, device="cpu"):
    run_case(case, kernels, device, modes=("whole",), places=fpt.PLACES[:1])
