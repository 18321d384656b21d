"""numpy restatement of the gradient-norm kernels' exact summation order. TEST INFRASTRUCTURE.

diloco-swarm_amd/csrc/dl_norm.hip, operation for operation (every sum in fp64; the square of an
fp32 value is exact in fp64, so there is no fma to emulate):

  lane t of the 256 of a chunk's workgroup:
      acc = 0; for u = 0..3, for k = 0..3 (x, y, z, w): the chunk's element 4*(u*256 + t) + k,
      where float4 u*256 + t lies inside len >> 2; then the tail element 4*(len >> 2) + t
  wave (64 lanes):  xor-butterfly, o = 32, 16, 8, 4, 2, 1: v += v[lane ^ o]
  workgroup:        ((w0 + w1) + w2) + w3 of the four waves -> partials[c]
  dl_norm_finish:   lane t sums partials[t], partials[t + 256], ...; the same butterfly and
                    four-wave sum; sqrt in fp64; norm = fp32(sqrt)
  coefficient:      torch's fp32 sequence for `max_norm / (norm + 1e-6)` with a Python float on
                    the left -- (norm + 1e-6f).reciprocal() * max_norm -- then clamp(max=1),
                    a NaN staying a NaN

Chunks are oracle.chunks_of of each tensor, in tensor order (the tree's chunk table)."""
import numpy as np

from oracle import oracle

THREADS, UNROLL, WAVE = 256, 4, 64
F32 = np.float32


def block_sum(lanes: np.ndarray) -> np.float64:
    """256 per-lane fp64 values -> the workgroup's sum, in the kernels' order."""
    v = np.asarray(lanes, dtype=np.float64).reshape(THREADS // WAVE, WAVE).copy()
    lane = np.arange(WAVE)
    with np.errstate(all="ignore"):
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[:, lane ^ o]
        w = v[:, 0]
        return ((w[0] + w[1]) + w[2]) + w[3]


def chunk_lanes(x: np.ndarray) -> np.ndarray:
    """Per-lane Σ g² of one chunk (fp32, 1..4096 elements), before the workgroup reduce."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = x.size
    assert 0 < n <= oracle.CHUNK
    nv = n >> 2
    with np.errstate(all="ignore"):
        d = x.astype(np.float64)
        sq = d * d  # exact
        # rows[u, t, k] = element 4*(u*256 + t) + k; rows past the chunk add +0.0, which leaves
        # an accumulator that starts at +0.0 and only ever receives squares unchanged
        rows = np.zeros(UNROLL * THREADS * 4, dtype=np.float64)
        rows[:4 * nv] = sq[:4 * nv]
        rows = rows.reshape(UNROLL, THREADS, 4)
        acc = np.zeros(THREADS, dtype=np.float64)
        for u in range(UNROLL):
            for k in range(4):
                acc = acc + rows[u, :, k]
        tail = sq[4 * nv:]
        acc[:tail.size] = acc[:tail.size] + tail
    return acc


def chunk_sumsq(x: np.ndarray) -> np.float64:
    return block_sum(chunk_lanes(x))


def tree_partials(tensors) -> np.ndarray:
    """partials[c] for every chunk of the tree, tensors in parameters() order."""
    out = []
    for t in tensors:
        t = np.ascontiguousarray(t, dtype=np.float32).reshape(-1)
        for o, n in oracle.chunks_of(t.size):
            out.append(chunk_sumsq(t[o:o + n]))
    return np.asarray(out, dtype=np.float64)


def finish(partials: np.ndarray, max_norm: float):
    """(norm, coef) as fp32 scalars, from the per-chunk partial sums."""
    p = np.asarray(partials, dtype=np.float64)
    rounds = -(-p.size // THREADS)
    pad = np.zeros(max(rounds, 1) * THREADS, dtype=np.float64)
    pad[:p.size] = p
    pad = pad.reshape(-1, THREADS)
    with np.errstate(all="ignore"):
        acc = np.zeros(THREADS, dtype=np.float64)
        for r in range(rounds):
            acc = acc + pad[r]
        norm = F32(np.sqrt(block_sum(acc)))
        c = (F32(1.0) / (norm + F32(1e-6))) * F32(max_norm)
    coef = c if c < 1 else (c if c != c else F32(1.0))
    return F32(norm), F32(coef)


def norm_and_coef(tensors, max_norm: float):
    return finish(tree_partials(tensors), max_norm)


def scaled(x: np.ndarray, coef) -> np.ndarray:
    """dl_scale_by: untouched when coef == 1, else the fp32 product (NaN / 0 multiply)."""
    x = np.asarray(x, dtype=np.float32)
    if coef == 1:
        return x.copy()
    with np.errstate(all="ignore"):
        return (x * F32(coef)).astype(np.float32)


def clip(tensors, max_norm: float):
    """(norm, coef, clipped tensors): clip_grad_norm_ as the device path computes it."""
    norm, coef = norm_and_coef(tensors, max_norm)
    return norm, coef, [scaled(t, coef) for t in tensors]
