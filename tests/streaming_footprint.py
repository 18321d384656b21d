"""Write-footprint rows of the two merging kernels, on the helpers of tests/footprint.py.
TEST HELPER.

footprint.Rig lays the buffers of a call out in one byte arena of sentinels and compares every
byte with the CPU reference after every launch: the padding of θ, the state and the wire, the
guard bands around every inner tensor, the wire itself (only read) and, in a single-bucket call,
the other buckets. The reference gains the merging stand-ins (tests/streaming_oracle_kernels.py)."""
import footprint as fpt
from diloco_amd.plan import SLOT_INNER
from streaming_oracle_kernels import MergeStandIns

ALPHAS = (0.5, 0.3)


class MergeFootprintKernels(MergeStandIns, fpt.FootprintKernels):
    pass


REF = MergeFootprintKernels()


class Rig(fpt.Rig):
    def commit(self, kernels=None, device="cpu", grids=(0,)):
        super().commit(kernels, device, grids)
        self.ref.K = REF  # the same tree and bindings, the backend that knows the merging calls


def run_case(case, kernels=None, device="cpu", grids=(0,), modes=fpt.MODES, places=None):
    """footprint.run_case on the Rig above."""
    for sentinel in fpt.SENTINELS:
        for place in places or case.places:
            for mode in modes:
                rig = Rig(sentinel, place)
                case.setup(rig)
                rig.commit(kernels, device, grids)
                try:
                    rig.run(case.steps, mode, inside=kernels is None, empty=case.empty)
                except AssertionError as e:
                    raise AssertionError(f"{case.name} [{sentinel} sentinel, placement {place}, "
                                         f"{mode}]: {e}") from None


def cases_unpack_sgd_merge(wire):
    """The first-step mode, new inner values, then the steady one; divisor 3. Both alphas with
    Nesterov, one each for the other two modes."""
    for k, (label, momentum, nesterov) in enumerate(fpt._sgd_modes()):
        for alpha in ALPHAS if nesterov else ALPHAS[k % 2:k % 2 + 1]:
            def call(first, momentum=momentum, nesterov=nesterov, alpha=alpha):
                return lambda K, T, S, b: K.unpack_sgd_merge(
                    T, b, S.wire, 3, S.theta, S.mom if momentum else None, fpt.LR, momentum,
                    nesterov, first, SLOT_INNER, alpha)
            yield fpt.Case(f"unpack_sgd_merge {wire}, {label}, alpha {alpha}",
                           fpt._buffers(*fpt._sgd_state(wire, True, bool(momentum))),
                           [call(True), fpt.Feed("inner"), fpt.Feed("wire"), call(False)])


def cases_unpack_adamw_merge(wire):
    for divisor, alpha in zip((1, 3), ALPHAS):
        def call(t, divisor=divisor, alpha=alpha):
            return lambda K, T, S, b: K.unpack_adamw_merge(
                T, b, S.wire, divisor, S.theta, S.m, S.v, fpt.ADAM[t], SLOT_INNER, alpha)
        yield fpt.Case(f"unpack_adamw_merge {wire}, divisor {divisor}, alpha {alpha}",
                       fpt._buffers(*fpt._adam_state(wire, True)),
                       [call(0), fpt.Feed("inner"), fpt.Feed("wire"), call(1)])


TREE_ROWS = {"unpack_sgd_merge": cases_unpack_sgd_merge,
             "unpack_adamw_merge": cases_unpack_adamw_merge}
