"""The top-k wires' all-gather exchange (include/diloco_hip.h) in numpy. TEST HELPER. Dense adds give
the sparse ones' bits: adding +0 never changes a finite value, and acc is never -0."""
import numpy as np

F, CHUNK = np.float32, 4096


def average_tensors(ref, slots_by_peer, k, numels):
    """ref: topk[_fp4]_restatement; every peer's slots of a whole tree -> the averaged tensors."""
    S = slots_by_peer[0].size // sum(-(-t // CHUNK) for t in numels)
    out, c, n = [], 0, len(slots_by_peer)
    for t in numels:
        dense = []
        for j in range(c, c - (-t // CHUNK)):
            acc = np.zeros(CHUNK, dtype=F)
            with np.errstate(all="ignore"):
                for p in slots_by_peer:
                    acc = acc + ref.decode(p[j * S:(j + 1) * S], k)
                dense.append(acc / F(n) if n > 1 else acc)
        out.append(np.concatenate(dense)[:t])
        c -= -t // CHUNK
    return out
