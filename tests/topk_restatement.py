"""The top-k sparse wire codec of include/diloco_hip.h in numpy: selection (a stable argsort of
the negated key, the first k, sorted by index), decode, the owner's reduce, and the two-stage
exchange with residuals. Every operation is one fp32 operation, as the header states it."""
import numpy as np
from fp4_restatement import same_bits  # noqa: F401  (bit-exact, NaNs by position)

F = np.float32
CHUNK = 4096


def select(x, k, ef):
    """x: one dense chunk of CHUNK fp32 -> (6k slot bytes, residual or None)."""
    key = x.view(np.uint32) & np.uint32(0x7FFFFFFF)
    idx = np.sort(np.argsort(-key.astype(np.int64), kind="stable")[:k])
    slot = np.concatenate([x[idx].view(np.uint8), idx.astype(np.uint16).view(np.uint8)])
    res = None
    if ef:
        res = x.copy()
        res[idx] = 0.0
    return slot, res


def decode(slot, k):
    out = np.zeros(CHUNK, dtype=np.uint32)
    out[slot[4 * k:].view(np.uint16)] = slot[:4 * k].view(np.uint32)
    return out.view(F)


def encode_tensor(x, k, res=None):
    """A tensor's chunks (+0 past its length) -> (its slots' bytes, its new residual or None);
    x = delta + res is one rounded add."""
    n = x.size
    if res is not None:
        x = x + res
    slots, out = [], []
    for o in range(0, n, CHUNK):
        c = np.zeros(CHUNK, dtype=F)
        c[:min(CHUNK, n - o)] = x[o:o + CHUNK]
        s, r = select(c, k, res is not None)
        slots.append(s)
        if r is not None:
            out.append(r[:min(CHUNK, n - o)])
    return np.concatenate(slots), (np.concatenate(out) if out else None)


def reduce_slots(recv, n, m, divisor, k, res=None):
    """recv laid out [peer][slot] -> (m averaged slots, the new residual of m·CHUNK or None)."""
    S = 6 * k
    out, new = [], []
    with np.errstate(all="ignore"):
        for j in range(m):
            acc = np.zeros(CHUNK, dtype=F)
            for r in range(n):
                s = recv[(r * m + j) * S:(r * m + j + 1) * S]
                for v, i in zip(s[:4 * k].view(F), s[4 * k:].view(np.uint16)):
                    acc[i] = acc[i] + v
            if divisor > 1:
                acc = acc / F(divisor)
            if res is not None:
                acc = acc + res[j * CHUNK:(j + 1) * CHUNK]
            s, r2 = select(acc, k, res is not None)
            out.append(s)
            new.append(r2)
    return np.concatenate(out), (np.concatenate(new) if res is not None else None)


class TopkExchange:
    """The exchange over a tree for n ranks: average(deltas_by_rank) encodes on every rank,
    all_to_all, reduces on every shard owner (divisor n), all_gather, decodes. State:
    enc[rank][tensor], red[bucket][owner]."""

    def __init__(self, numels, bucket_chunks, n, k, ef=True):
        self.numels, self.bucket_chunks, self.n, self.k, self.ef = numels, bucket_chunks, n, k, ef
        self.enc = [[np.zeros(t, dtype=F) for t in numels] for _ in range(n)]
        self.red = [[np.zeros(-(-nch // n) * CHUNK, dtype=F) for _ in range(n)]
                    for nch in bucket_chunks]

    def average(self, deltas_by_rank):
        n, k, S = self.n, self.k, 6 * self.k
        slots = []
        for r in range(n):
            per = []
            for t, d in enumerate(deltas_by_rank[r]):
                s, res = encode_tensor(d, k, self.enc[r][t] if self.ef else None)
                if self.ef:
                    self.enc[r][t] = res
                per.append(s)
            slots.append(np.concatenate(per))
        avg, c = [], 0
        for b, nch in enumerate(self.bucket_chunks):
            m = -(-nch // n)
            per = [np.concatenate([slots[r][c * S:(c + nch) * S],
                                   np.zeros((n * m - nch) * S, dtype=np.uint8)]) for r in range(n)]
            got = []
            for p in range(n):  # peer p owns slots [p*m, (p+1)*m) of every rank's region
                recv = np.concatenate([per[r][p * m * S:(p + 1) * m * S] for r in range(n)])
                red, res = reduce_slots(recv, n, m, n, k, self.red[b][p] if self.ef else None)
                if self.ef:
                    self.red[b][p] = res
                got.append(red)
            avg.append(np.concatenate(got)[:nch * S])
            c += nch
        flat = np.concatenate(avg)
        out, c = [], 0
        for t in self.numels:
            nch = -(-t // CHUNK)
            dense = [decode(flat[(c + j) * S:(c + j + 1) * S], k) for j in range(nch)]
            out.append(np.concatenate(dense)[:t])
            c += nch
        return out
