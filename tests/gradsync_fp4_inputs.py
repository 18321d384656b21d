"""Inputs of the fp4 gradient-sync tests (CPU and GPU). TEST HELPER.

NUMELS (bucket cap 4096): a 1-element chunk, tails under 4 and under 32, a chunk one short of
full, a full one, a one-element spill into a second chunk, a three-chunk tensor; several buckets.
groupwise(): every group of 32 at its own magnitude, so groups carry different E; one element per
group near the group's amax and the others below half a quantiser step, so most elements decode
to 0 and live on in the residual. special(): on top of that the tie values in a group with amax 6,
a negative zero, a group of denormals, one NaN group and one Inf group."""
import numpy as np

F = np.float32
NUMELS = [1, 3, 31, 33, 257, 4095, 4096, 4097, 8197]
CAP = 4096
TIES = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]


def groupwise(seed, numels=NUMELS, lo=-3.0, hi=0.0):
    rng = np.random.default_rng(seed)
    out = []
    for n in numels:
        g = -(-n // 32)
        mag = np.repeat(10.0 ** rng.uniform(lo, hi, g), 32)[:n]
        x = mag * 0.02 * rng.standard_normal(n)
        big = np.arange(g) * 32 + rng.integers(0, 32, g)
        big = big[big < n]
        x[big] = mag[big] * rng.uniform(0.5, 1.0, big.size) * rng.choice([-1.0, 1.0], big.size)
        out.append(x.astype(F))
    return out


def special(seed, numels=NUMELS):
    """groupwise() with the special values planted; tensor 6 (4096) and 8 (8197) carry them."""
    out = groupwise(seed, numels)
    a = out[numels.index(4096)]
    a[0:32] = 0.0
    a[0] = 6.0  # E = 127: y = |x|, the ties go to the even code
    a[1:8] = TIES
    a[8:15] = [-t for t in TIES]
    a[15] = -0.0
    a[64:96] = (np.random.default_rng(seed + 1).standard_normal(32) * 1e-40).astype(F)  # denormals
    a[128 + 5] = np.nan
    b = out[numels.index(8197)]
    b[4096 + 40] = np.inf
    b[8197 - 2] = -0.0  # in the < 4 tail of the last chunk
    return out
