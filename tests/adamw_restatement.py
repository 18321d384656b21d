"""The AdamW outer step restated in numpy, for whole trees. TEST INFRASTRUCTURE.

One element of torch's `_single_tensor_adamw` (amsgrad, maximize, capturable off; beta1 > 0.5)
as this torch build's CPU kernels round it, which is the arithmetic contract of dl_unpack_adamw
and dl_delta_pack_adamw (include/diloco_hip.h). The host scalars are Python doubles, written
as torch writes them, each narrowed to fp32 once:

    g  = wire / divisor          (IEEE division; divisor 1: untouched; bf16 wire widened first)
    th = th * decay                                   decay = 1 - lr*wd
    m  = fma(w1, g - m, m)                            w1 = 1 - beta1
    v  = v * beta2 ;  v = fma(w2 * g, g, v)           w2 = 1 - beta2
    den = sqrtf(v) / bs + eps                         bs = (1 - beta2**t) ** 0.5
    th = th + (nss * m) / den                         nss = -(lr / (1 - beta1**t))

Every fp32 operation is numpy's (IEEE, correctly rounded, denormals kept); the two fmas are
exact: `fmaf` below forms a*b exactly in fp64, adds c with an error-free TwoSum, and rounds
the pair to odd before the single narrowing to fp32 (a 53-bit round-to-odd value narrows to 24
bits as the exact sum would). tests/test_adamw_cpu.py pins it against libm's fmaf.
"""
import ctypes
import ctypes.util

import numpy as np

F = np.float32


def fmaf(a, b, c) -> np.ndarray:
    """fma(a, b, c) in fp32 with one rounding, elementwise."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F))
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)  # exact: 24 + 24 bits
        c = c.astype(np.float64)
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)  # TwoSum: s + e == p + c exactly
        bits = s.view(np.int64).copy()
        fix = (e != 0) & ((bits & 1) == 0) & np.isfinite(s)
        up = (e > 0) == (s > 0)  # away from zero: the bit pattern grows
        bits[fix & up] += 1
        bits[fix & ~up] -= 1
        return bits.view(np.float64).astype(F)


def libm_fmaf():
    """libm's fmaf through ctypes (one call per element: the check of `fmaf` above)."""
    lib = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    f = lib.fmaf
    f.restype = ctypes.c_float
    f.argtypes = [ctypes.c_float] * 3
    return f


def bf16_round(x: np.ndarray) -> np.ndarray:
    """fp32 -> bf16 (round to nearest even) -> fp32, finite values."""
    u = np.ascontiguousarray(x, F).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(F)


def scalars(lr, betas, weight_decay, eps, t):
    """(decay, w1, beta2, w2, nss, bs, eps) as fp32, from doubles written as torch writes them."""
    beta1, beta2 = betas
    t = float(t)  # torch reads the step count from its fp32 scalar tensor: a float exponent
    bias_correction1 = 1 - beta1 ** t
    bias_correction2 = 1 - beta2 ** t
    step_size = lr / bias_correction1
    return tuple(F(x) for x in (1 - lr * weight_decay, 1 - beta1, beta2, 1 - beta2, -step_size,
                                bias_correction2 ** 0.5, eps))


def adamw_elementwise(th, m, v, g, sc):
    """One step on fp32 arrays (returned new): g is the gradient as the optimizer sees it."""
    decay, w1, beta2, w2, nss, bs, eps = sc
    assert all(x.dtype == F for x in (th, m, v, g))
    with np.errstate(all="ignore"):
        th = th * decay
        m = fmaf(w1, g - m, m)
        v = v * beta2
        v = fmaf(w2 * g, g, v)
        den = np.sqrt(v) / bs + eps
        th = th + (nss * m) / den
    return th, m, v


class AdamWState:
    """A tree's outer AdamW state (lists of flat fp32 arrays) stepped as the four calls step it:
    delta per rank (a bf16 wire rounds it), Σ in rank order, / n, AdamW, inner = θ."""

    def __init__(self, theta, lr=0.01, betas=(0.9, 0.95), weight_decay=0.1, eps=1e-8):
        self.theta = [np.array(t, F).reshape(-1) for t in theta]
        self.m = [np.zeros_like(t) for t in self.theta]
        self.v = [np.zeros_like(t) for t in self.theta]
        self.lr, self.betas, self.wd, self.eps = lr, betas, weight_decay, eps
        self.t = 0

    def step_grads(self, grads):
        self.t += 1
        sc = scalars(self.lr, self.betas, self.wd, self.eps, self.t)
        for i, g in enumerate(grads):
            self.theta[i], self.m[i], self.v[i] = adamw_elementwise(
                self.theta[i], self.m[i], self.v[i], np.asarray(g, F).reshape(-1), sc)

    def step(self, inners_by_rank, wire="f32", divisor=None):
        """Returns (deltas[rank][tensor] as they sit on the wire, the averaged gradients)."""
        n = len(inners_by_rank)
        deltas = []
        for inner in inners_by_rank:
            d = [t - np.asarray(x, F).reshape(-1) for t, x in zip(self.theta, inner)]
            deltas.append([bf16_round(x) for x in d] if wire == "bf16" else d)
        avg = []
        for i in range(len(self.theta)):
            s = deltas[0][i]
            for r in range(1, n):
                s = s + deltas[r][i]
            if wire == "bf16" and n > 1:
                s = bf16_round(s)  # the collective's bf16 SUM
            div = n if divisor is None else divisor
            avg.append(s if div == 1 else s / F(div))
        self.step_grads(avg)
        return deltas, avg
