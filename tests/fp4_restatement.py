"""The 4-bit (MXFP4) wire codec, restated in numpy only. TEST HELPER.

Slot (SLOT = 2176 bytes per 4096-element chunk): bytes [0, 128) one scale byte E per group of 32
elements, bytes [128, 2176) the payload, element i in byte 128 + i//2, low nibble for even i.
A nibble is sign << 3 | code, code indexing GRID. Elements past the chunk's length count as +0.

Scale of a group, A = max(bits(x) & 0x7fffffff) as an unsigned integer:
    A >= 0x7f800000            E = 255, every nibble 0
    A == 0                     E = 0, every nibble 0
    else amax = m * 2^k, m in [0.5, 1) (frexp): e = k - 3 if m <= 0.75 else k - 2,
                               E = max(0, e + 127)
Element: y = |x| * 2^(127 - E) (exact, in doubles), code = the grid point nearest y, ties to the
even code; the sign bit only where code != 0.
Decode: E == 255 -> NaN; else +-GRID[code] * 2^(E - 127), exact in fp32 (denormals included).

Error feedback and the reduce follow tests/q8_ef_restatement.py's statements with this codec:
    encoder  x = (θ - inner) + r;  slot = enc(x);  r' = x - deq(slot)
    reduce   acc = 0; acc = acc + deq_r in rank order; / divisor when > 1; (+ r2;) re-encode
Fp4Exchange composes both into one outer step's exchange over a tree, as EFExchange does."""
import numpy as np

CHUNK, GROUP = 4096, 32
N_GROUPS = CHUNK // GROUP  # 128 scale bytes
SLOT = N_GROUPS + CHUNK // 2  # 2176
GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=np.float64)
TWICE = np.array([0, 1, 2, 3, 4, 6, 8, 12], dtype=np.int64)  # 2 * GRID, as integers
F = np.float32


def chunks_of(numel):
    return [(o, min(CHUNK, numel - o)) for o in range(0, numel, CHUNK)]


def group_scales(x: np.ndarray) -> np.ndarray:
    """E per group of 32 for x of CHUNK fp32 values."""
    a = (np.ascontiguousarray(x, dtype=F).view(np.uint32) & np.uint32(0x7FFFFFFF))
    a = a.reshape(-1, GROUP).max(axis=1)
    with np.errstate(all="ignore"):
        m, k = np.frexp(a.view(F).astype(np.float64))  # denormals are values like any other
    e = np.where(m <= 0.75, k - 3, k - 2)
    big = np.maximum(0, e + 127)
    return np.where(a >= 0x7F800000, 255, np.where(a == 0, 0, big)).astype(np.uint8)


def nearest_codes(y: np.ndarray) -> np.ndarray:
    """The code of the grid point nearest y >= 0, ties to the even code."""
    d = np.abs(y[:, None] - GRID[None, :])
    lo = d.argmin(axis=1)
    hi = GRID.size - 1 - d[:, ::-1].argmin(axis=1)
    return np.where(lo % 2 == 0, lo, hi).astype(np.uint8)


def encode_values(x: np.ndarray) -> np.ndarray:
    """One chunk's fp32 values x (len <= CHUNK) -> its slot."""
    n = x.size
    assert 0 <= n <= CHUNK
    v = np.zeros(CHUNK, dtype=F)
    v[:n] = x
    e = group_scales(v)
    per = np.repeat(e.astype(np.int64), GROUP)
    live = per != 255
    nib = np.zeros(CHUNK, dtype=np.uint8)
    with np.errstate(all="ignore"):
        y = np.ldexp(np.abs(v[live]).astype(np.float64), (127 - per[live]).astype(np.int64))
    code = nearest_codes(y)
    neg = np.signbit(v[live]) & (code != 0)  # a negative zero is never emitted
    nib[live] = code | (neg.astype(np.uint8) << 3)
    slot = np.empty(SLOT, dtype=np.uint8)
    slot[:N_GROUPS] = e
    slot[N_GROUPS:] = nib[0::2] | (nib[1::2] << 4)
    return slot


def decode_slot(slot: np.ndarray, n: int = CHUNK) -> np.ndarray:
    """The first n values a slot holds."""
    slot = np.asarray(slot, dtype=np.uint8)
    assert slot.size == SLOT
    per = np.repeat(slot[:N_GROUPS].astype(np.int64), GROUP)
    nib = np.empty(CHUNK, dtype=np.uint8)
    nib[0::2] = slot[N_GROUPS:] & 15
    nib[1::2] = slot[N_GROUPS:] >> 4
    t = TWICE[nib & 7] * np.where(nib & 8, -1, 1)  # nibble 8 (never emitted) decodes to +0
    out = np.ldexp(t.astype(np.float64), per - 128).astype(F)  # exact: 2^-128 is a denormal
    out[per == 255] = np.nan
    return out[:n]


def quantise_with_residual(x: np.ndarray):
    """(slot, x - deq(slot)) for one chunk's fp32 values x (len <= CHUNK)."""
    x = np.ascontiguousarray(x, dtype=F)
    slot = encode_values(x)
    with np.errstate(all="ignore"):
        return slot, (x - decode_slot(slot, x.size)).astype(F)


def encode_chunk(theta: np.ndarray, inner: np.ndarray, r=None):
    """dl_delta_fp4 on one chunk: (slot, new residual or None)."""
    with np.errstate(all="ignore"):
        x = (theta.astype(F) - inner.astype(F)).astype(F)
        if r is None:
            return encode_values(x), None
        x = (x + r.astype(F)).astype(F)
    return quantise_with_residual(x)


def encode_delta(delta: np.ndarray, r=None):
    """One tensor's pseudo-gradient already formed: (its slots, its new residual or None)."""
    slots, out = [], None if r is None else np.empty_like(r)
    for o, n in chunks_of(delta.size):
        s, rr = encode_chunk(delta[o:o + n], np.zeros(n, dtype=F), None if r is None else r[o:o + n])
        if r is not None:
            out[o:o + n] = rr
        slots.append(s)
    return (np.concatenate(slots) if slots else np.zeros(0, dtype=np.uint8)), out


def reduce_slots(recv: np.ndarray, n: int, m: int, divisor: int, r2=None):
    """dl_fp4_reduce: recv holds n x m slots ([peer][slot]); (m averaged slots, new r2 or None)."""
    out = np.zeros(m * SLOT, dtype=np.uint8)
    res = None if r2 is None else np.empty(m * CHUNK, dtype=F)
    for j in range(m):
        acc = np.zeros(CHUNK, dtype=F)
        with np.errstate(all="ignore"):
            for r in range(n):
                acc = (acc + decode_slot(recv[(r * m + j) * SLOT:(r * m + j + 1) * SLOT])).astype(F)
            if divisor > 1:
                acc = (acc / F(divisor)).astype(F)
            if r2 is not None:
                acc = (acc + r2[j * CHUNK:(j + 1) * CHUNK]).astype(F)
        if r2 is None:
            out[j * SLOT:(j + 1) * SLOT] = encode_values(acc)
        else:
            out[j * SLOT:(j + 1) * SLOT], res[j * CHUNK:(j + 1) * CHUNK] = \
                quantise_with_residual(acc)
    return out, res


def decode_tensors(flat: np.ndarray, numels):
    """A tree's slots in chunk order -> one fp32 array per tensor."""
    out, c = [], 0
    for numel in numels:
        parts = [decode_slot(flat[(c + j) * SLOT:(c + j + 1) * SLOT], n)
                 for j, (_o, n) in enumerate(chunks_of(numel))]
        out.append(np.concatenate(parts) if parts else np.zeros(0, dtype=F))
        c += len(parts)
    return out


class Fp4Exchange:
    """The fp4 exchange over a tree for n ranks, composed as q8_ef_restatement.EFExchange is:
    average(deltas_by_rank) encodes on every rank, all_to_all, reduces on every shard owner
    (divisor n), all_gather, decodes. ef: both stages carry their residual. State:
    enc[rank][tensor], red[bucket][owner]; avg_slots: the averaged slots per bucket."""

    def __init__(self, numels, bucket_chunks, n, ef=True):
        self.numels, self.bucket_chunks, self.n, self.ef = list(numels), list(bucket_chunks), n, ef
        self.enc = [[np.zeros(k, dtype=F) for k in numels] for _ in range(n)]
        self.red = [[np.zeros(-(-nch // n) * CHUNK, dtype=F) for _ in range(n)]
                    for nch in bucket_chunks]
        self.avg_slots = None

    def average(self, deltas_by_rank):
        n = self.n
        slots = []
        for r in range(n):
            per = []
            for t in range(len(self.numels)):
                s, res = encode_delta(deltas_by_rank[r][t], self.enc[r][t] if self.ef else None)
                if self.ef:
                    self.enc[r][t] = res
                per.append(s)
            slots.append(np.concatenate(per))
        avg_slots, c = [], 0
        for b, nch in enumerate(self.bucket_chunks):
            m = -(-nch // n)
            per = []
            for r in range(n):
                s = np.zeros(n * m * SLOT, dtype=np.uint8)
                s[:nch * SLOT] = slots[r][c * SLOT:(c + nch) * SLOT]
                per.append(s)
            gathered = []
            for p in range(n):  # all_to_all: peer p gets slots [p*m, (p+1)*m) from every rank
                recv = np.concatenate([per[r][p * m * SLOT:(p + 1) * m * SLOT] for r in range(n)])
                red, res = reduce_slots(recv, n, m, n, self.red[b][p] if self.ef else None)
                if self.ef:
                    self.red[b][p] = res
                gathered.append(red)
            avg_slots.append(np.concatenate(gathered)[:nch * SLOT])
            c += nch
        self.avg_slots = avg_slots
        return decode_tensors(np.concatenate(avg_slots), self.numels)


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    """Bit-exact, NaNs compared by position (their payload is not part of the contract)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    return a[~na].tobytes() == b[~nb].tobytes()
