"""Write-footprint rows of dl_gather_fp4 and dl_unpack_avg_fp4, on the Rig of
tests/fp4_footprint.py (tests/footprint.py's arena, sentinels and comparison). TEST HELPER.

The reference is the checker backend with the two stand-ins of
tests/gradsync_fp4_oracle_kernels.py. gather_fp4: the gradients are only read, every byte of every
launched slot is written (`dirty`: garbage in them beforehand, on the copies under test only), no
other slot, and of the residual nothing outside the segments. unpack_avg_fp4: the slots (written
by gather_fp4 on the same rig from a second set of tensors, so every copy decodes equal bytes)
are only read, nothing is stored outside the destination tensors, and the partials are written
for exactly the launch's chunk range."""
import footprint as fpt
import fp4_footprint as f4
from diloco_amd.plan import SLOT_AUX, SLOT_GRAD
from gradsync_fp4_oracle_kernels import GradFp4StandIns


class GradFp4FootprintKernels(GradFp4StandIns, f4.Fp4FootprintKernels):
    pass


REF = GradFp4FootprintKernels()


class Rig(f4.Rig):
    def commit(self, kernels=None, device="cpu", grids=(0,)):
        super().commit(kernels, device, grids)
        self.ref.K = REF  # the same tree and bindings, the backend that knows the two calls


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


def _gather(ef, dirty=False, slot=SLOT_GRAD):
    def call(K, T, S, b):
        if dirty:
            f4._dirty(S, f4.slots_of(S, "slots", b))
        K.gather_fp4(T, b, slot, S.resid if ef else None, f4.slots_of(S, "slots", b))
    return call


def cases_gather_fp4(ef):
    specs = [("slot", "grads", SLOT_GRAD), ("fp4", "slots")]
    if ef:
        specs.append(("packed", "resid", {"fill": "small"}))
    for dirty in (False, True):
        yield fpt.Case(f"gather_fp4{' with residual' if ef else ''}{', dirty slots' if dirty else ''}",
                       fpt._buffers(*specs), [_gather(ef, dirty), fpt.Feed("grads"),
                                              _gather(ef, dirty)])


def cases_unpack_avg_fp4(sumsq):
    specs = [("slot", "grads", SLOT_GRAD), ("slot", "peer", SLOT_AUX, 1), ("fp4", "slots")]
    if sumsq:
        specs.append(("partials", "partials"))

    def call(K, T, S, b):
        K.unpack_avg_fp4(T, b, f4.slots_of(S, "slots", b), SLOT_GRAD,
                         S.partials if sumsq else None)
    enc = _gather(False, slot=SLOT_AUX)
    yield fpt.Case(f"unpack_avg_fp4{' with partials' if sumsq else ''}", fpt._buffers(*specs),
                   [enc, call, fpt.Feed("peer"), enc, call])


ROWS = {
    "gather_fp4": lambda: cases_gather_fp4(False), "gather_fp4_ef": lambda: cases_gather_fp4(True),
    "unpack_avg_fp4": lambda: cases_unpack_avg_fp4(False),
    "unpack_avg_fp4_sumsq": lambda: cases_unpack_avg_fp4(True),
}
