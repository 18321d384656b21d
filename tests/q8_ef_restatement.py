"""Error feedback on the int8 wire, restated in numpy on top of the C oracle. TEST HELPER.

The encoder with a residual (dl_delta_q8_ef), per chunk:
    x = (θ - inner) + r                 two fp32 operations, each rounded
    slot = or_delta_q8(x, zeros)        the oracle's quantiser, exact because x - 0 = x
    r' = x - or_q8_deq(slot)            float(q) * s, then one subtract
The reduce with a residual (dl_q8_reduce_ef), per slot j of the owner: the sum of the peers'
dequantised slots in rank order as or_q8_reduce forms it (acc = 0; acc = acc + deq_r; / divisor
when > 1), then the same residual step on all 4096 values.
EFExchange composes both into one outer step's exchange over a tree, as oracle.q8_average does
for the plain codec. Non-finite values follow IEEE rules, as in the kernels."""
import numpy as np

from oracle import oracle

Q8_SLOT, CHUNK = oracle.Q8_SLOT, oracle.CHUNK


def quantise_with_residual(x: np.ndarray):
    """(slot, x - deq(slot)) for one chunk's fp32 values x (len <= CHUNK)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = x.size
    slot = np.zeros(Q8_SLOT, dtype=np.uint8)
    deq = np.empty(n, dtype=np.float32)
    lib = oracle.load()
    lib.or_delta_q8(oracle._fp(x), oracle._fp(np.zeros(n, dtype=np.float32)), n, oracle._u8(slot))
    lib.or_q8_deq(oracle._u8(slot), n, oracle._fp(deq))
    with np.errstate(all="ignore"):
        return slot, (x - deq).astype(np.float32)


def encode_chunk(theta: np.ndarray, inner: np.ndarray, r: np.ndarray):
    """dl_delta_q8_ef on one chunk: (slot, new residual)."""
    with np.errstate(all="ignore"):
        d = (theta.astype(np.float32) - inner.astype(np.float32)).astype(np.float32)
        x = (d + r.astype(np.float32)).astype(np.float32)
    return quantise_with_residual(x)


def encode_delta(delta: np.ndarray, r: np.ndarray):
    """One tensor's pseudo-gradient already formed: (its slots, its new residual)."""
    slots, out = [], np.empty_like(r)
    for o, n in oracle.chunks_of(delta.size):
        s, out[o:o + n] = encode_chunk(delta[o:o + n], np.zeros(n, dtype=np.float32), r[o:o + n])
        slots.append(s)
    return np.concatenate(slots), out


def reduce_slots(recv: np.ndarray, n: int, m: int, divisor: int, r2: np.ndarray):
    """dl_q8_reduce_ef: recv holds n x m slots ([peer][slot]); (m averaged slots, new r2)."""
    out = np.zeros(m * Q8_SLOT, dtype=np.uint8)
    res = np.empty(m * CHUNK, dtype=np.float32)
    lib = oracle.load()
    for j in range(m):
        acc = np.zeros(CHUNK, dtype=np.float32)
        x = np.empty(CHUNK, dtype=np.float32)
        with np.errstate(all="ignore"):
            for r in range(n):
                slot = np.ascontiguousarray(recv[(r * m + j) * Q8_SLOT:(r * m + j + 1) * Q8_SLOT])
                lib.or_q8_deq(oracle._u8(slot), CHUNK, oracle._fp(x))
                acc = (acc + x).astype(np.float32)
            if divisor > 1:
                acc = (acc / np.float32(divisor)).astype(np.float32)
            v = (acc + r2[j * CHUNK:(j + 1) * CHUNK]).astype(np.float32)
        out[j * Q8_SLOT:(j + 1) * Q8_SLOT], res[j * CHUNK:(j + 1) * CHUNK] = \
            quantise_with_residual(v)
    return out, res


class EFExchange:
    """The int8 exchange with both residuals over a tree, for n ranks: average(deltas_by_rank)
    is oracle.q8_average with dl_delta_q8_ef on every rank and dl_q8_reduce_ef on every shard
    owner. n == 1 with reduce_ef=False is the one-replica engine: the encoder's residual and the
    plain in-place reduce. State: enc[rank][tensor], red[bucket][owner]."""

    def __init__(self, numels, bucket_chunks, n, reduce_ef=True):
        self.numels, self.bucket_chunks, self.n = list(numels), list(bucket_chunks), n
        self.reduce_ef = reduce_ef
        self.enc = [[np.zeros(k, dtype=np.float32) for k in numels] for _ in range(n)]
        self.red = [[np.zeros(-(-nch // n) * CHUNK, dtype=np.float32) for _ in range(n)]
                    for nch in bucket_chunks]

    def average(self, deltas_by_rank):
        n = self.n
        slots = []
        for r in range(n):
            per = []
            for t in range(len(self.numels)):
                s, self.enc[r][t] = encode_delta(deltas_by_rank[r][t], self.enc[r][t])
                per.append(s)
            slots.append(np.concatenate(per))
        avg_slots, c = [], 0
        for b, nch in enumerate(self.bucket_chunks):
            m = -(-nch // n)
            per = []
            for r in range(n):
                s = np.zeros(n * m * Q8_SLOT, dtype=np.uint8)
                s[:nch * Q8_SLOT] = slots[r][c * Q8_SLOT:(c + nch) * Q8_SLOT]
                per.append(s)
            gathered = []
            for p in range(n):  # all_to_all: peer p gets slots [p*m, (p+1)*m) from every rank
                recv = np.concatenate([per[r][p * m * Q8_SLOT:(p + 1) * m * Q8_SLOT]
                                       for r in range(n)])
                if self.reduce_ef:
                    red, self.red[b][p] = reduce_slots(recv, n, m, n, self.red[b][p])
                else:
                    red = oracle.q8_reduce(recv, n, m, n)
                gathered.append(red)
            avg_slots.append(np.concatenate(gathered)[:nch * Q8_SLOT])
            c += nch
        flat = np.concatenate(avg_slots)
        out, c = [], 0
        for numel in self.numels:
            k = len(oracle.chunks_of(numel))
            out.append(oracle.q8_deq(flat[c * Q8_SLOT:(c + k) * Q8_SLOT], numel))
            c += k
        return out


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    """Bit-exact, NaNs compared by position (their payload is not part of the contract)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    return a[~na].tobytes() == b[~nb].tobytes()
