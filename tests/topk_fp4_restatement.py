"""The top-k wire with 4-bit values (include/diloco_hip.h) in numpy: topk_restatement.select picks
the entries from the exact values; they are then quantised as the first k elements of an fp4 chunk
(fp4_restatement.encode_values: one scale per 32 consecutive entries, its nearest-even codes), so
the scale and code rules are the fp4 wire's own. Slot: 8 scale bytes, 8 zero bytes, k u16 entries
index | nibble << 12. Every operation is one fp32 operation, as the header states it."""
import numpy as np

import fp4_restatement as f4
import topk_restatement as tk
from fp4_restatement import same_bits  # noqa: F401  (bit-exact, NaNs by position)

F = np.float32
CHUNK = tk.CHUNK


def slot_bytes(k):
    return 16 + 2 * k


def select(x, k, ef):
    """x: one dense chunk of CHUNK fp32 -> (16 + 2k slot bytes, residual or None)."""
    s = tk.select(x, k, False)[0]
    val, idx = s[:4 * k].view(F), s[4 * k:].view(np.uint16)
    q = f4.encode_values(val)  # scale bytes [0, 8) are the entry groups', the rest stay 0
    pay = q[f4.N_GROUPS:f4.N_GROUPS + k // 2]
    nib = np.stack([pay & 15, pay >> 4], axis=1).reshape(-1).astype(np.uint16)
    slot = np.zeros(slot_bytes(k), dtype=np.uint8)
    slot[:8] = q[:8]
    slot[16:] = (idx | (nib << 12)).astype(np.uint16).view(np.uint8)
    res = None
    if ef:
        res = x.copy()
        with np.errstate(all="ignore"):
            res[idx] = val - f4.decode_slot(q, k)
    return slot, res


def entries(slot, k):
    """A slot's k (index, decoded value) pairs."""
    ent = slot[16:16 + 2 * k].view(np.uint16)
    e = np.repeat(slot[:8].astype(np.int64), 32)[:k]
    nib = (ent >> 12).astype(np.int64)
    t = f4.TWICE[nib & 7] * np.where(nib & 8, -1, 1)
    val = np.ldexp(t.astype(np.float64), e - 128).astype(F)  # exact: 2^-128 is a denormal
    val[e == 255] = np.nan
    return ent & 4095, val


def decode(slot, k):
    out = np.zeros(CHUNK, dtype=F)
    idx, val = entries(slot, k)
    out[idx] = val
    return out


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
    S = slot_bytes(k)
    out, new = [], []
    with np.errstate(all="ignore"):
        for j in range(m):
            acc = np.zeros(CHUNK, dtype=F)
            for r in range(n):
                s = recv[(r * m + j) * S:(r * m + j + 1) * S]
                idx, val = entries(s, k)
                acc[idx] = acc[idx] + val  # distinct indices (or k times 0 + 0 at index 0)
            if divisor > 1:
                acc = acc / F(divisor)
            if res is not None:
                acc = acc + res[j * CHUNK:(j + 1) * CHUNK]
            s, r2 = select(acc, k, res is not None)
            out.append(s)
            new.append(r2)
    return np.concatenate(out), (np.concatenate(new) if res is not None else None)


class TopkExchange(tk.TopkExchange):
    """topk_restatement.TopkExchange's two-stage exchange and state under this codec."""

    def average(self, deltas_by_rank):
        n, k, S = self.n, self.k, slot_bytes(self.k)
        slots = []
        for r in range(n):
            per = [encode_tensor(d, k, self.enc[r][t] if self.ef else None)
                   for t, d in enumerate(deltas_by_rank[r])]
            if self.ef:
                self.enc[r] = [res for _, res in per]
            slots.append(np.concatenate([s for s, _ in per]))
        dense, c = [], 0
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
            avg = np.concatenate(got)
            dense += [decode(avg[j * S:(j + 1) * S], k) for j in range(nch)]
            c += nch
        out, c = [], 0
        for t in self.numels:
            nch = -(-t // CHUNK)
            out.append(np.concatenate(dense[c:c + nch])[:t])
            c += nch
        return out
