"""The fp4 wire's randomised Hadamard rotation (include/diloco_hip.h states it), restated in numpy
only: sign, rotate, unrotate, vectorised per stage in fp32. TEST HELPER. Encode, decode and the
residual are composed with tests/fp4_restatement.py."""
import numpy as np

import fp4_restatement as fp4

CHUNK, BLOCK = fp4.CHUNK, 256
F = np.float32


def sign(seed: int) -> np.ndarray:
    """sigma of every position of a chunk, as booleans."""
    h = (np.arange(CHUNK, dtype=np.uint64) + np.uint64(seed)) & np.uint64(0xFFFFFFFF)
    for mul, shift in ((0x9E3779B1, 15), (0x85EBCA77, 13), (0xC2B2AE3D, 16)):
        h = (h * np.uint64(mul)) & np.uint64(0xFFFFFFFF)
        h ^= h >> np.uint64(shift)
    return (h >> np.uint64(31)).astype(bool)


def _flip(x: np.ndarray, seed: int) -> np.ndarray:
    bits = np.ascontiguousarray(x, dtype=F).view(np.uint32) ^ (sign(seed).astype(np.uint32) << 31)
    return bits.view(F)


def _stages(v: np.ndarray) -> np.ndarray:
    v = v.reshape(-1, BLOCK).astype(F)
    with np.errstate(all="ignore"):
        for s in range(8):
            w = v.reshape(-1, BLOCK >> (s + 1), 2, 1 << s)  # [.., bit s, low bits]
            a, b = w[:, :, 0, :].copy(), w[:, :, 1, :].copy()
            w[:, :, 0, :], w[:, :, 1, :] = a + b, a - b
        return (v * F(0.0625)).reshape(-1)


def rotate(x: np.ndarray, seed: int) -> np.ndarray:
    """R over one chunk's values x (len <= CHUNK): all CHUNK rotated positions."""
    v = np.zeros(CHUNK, dtype=F)
    v[:x.size] = x
    return _stages(_flip(v, seed))


def unrotate(y: np.ndarray, seed: int, n: int = CHUNK) -> np.ndarray:
    """The first n values of R^-1 over a chunk's CHUNK rotated values."""
    return _flip(_stages(np.asarray(y, dtype=F)), seed)[:n]


def encode_chunk(theta, inner, seed, r=None):
    """dl_delta_fp4_rot on one chunk: (slot, new residual or None)."""
    with np.errstate(all="ignore"):
        x = (theta.astype(F) - inner.astype(F)).astype(F)
        if r is not None:
            x = (x + r.astype(F)).astype(F)
        slot = fp4.encode_values(rotate(x, seed))
        return slot, None if r is None else (x - decode_chunk(slot, seed, x.size)).astype(F)


def decode_chunk(slot, seed, n=CHUNK):
    return unrotate(fp4.decode_slot(slot), seed, n)
