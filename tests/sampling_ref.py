"""Numpy restatement of the sampling contract of include/dglmi.h (DGLMISampleNeighbors,
DGLMICsrGatherRows, DGLMIBlockRelabel*), written from the header text, not from the kernels.
Shared by test_sampling_cpu.py and test_sampling_gpu.py."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays holding 32-bit values (Salmon et al., SC'11)."""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & MASK for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0) & MASK, np.uint64(k1) & MASK
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2  # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> S32, p0 & MASK, p1 >> S32, p1 & MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def draws(rng_seed, rng_ctr, slots, fanout):
    """r(i, t) for every slot i of ``slots`` and t < fanout: (len(slots), fanout) uint64."""
    slots = np.asarray(slots, np.uint64).reshape(-1, 1)
    t = np.arange(max(fanout, 1), dtype=np.uint64).reshape(1, -1)
    c = (np.uint64(rng_ctr) + (t >> np.uint64(2)))  # mod 2^64 by uint64 wrap
    c = np.broadcast_to(c, (slots.shape[0], t.shape[1]))
    s = np.broadcast_to(slots, c.shape)
    seed = np.uint64(rng_seed)
    out = philox4x32_10(c & MASK, c >> S32, s & MASK, s >> S32, seed & MASK, seed >> S32)
    comp = np.broadcast_to(t & np.uint64(3), c.shape)
    r = np.choose(comp.astype(np.int64), out)
    return r[:, :fanout]


def mulhi(r, n):
    return int((int(r) * int(n)) >> 32)


def pick_positions(r, deg, fanout, replace):
    """The sorted picks (positions inside the row) of one seed from its draws ``r``."""
    if deg == 0 or fanout == 0:
        return []
    if replace:
        return sorted(mulhi(r[t], deg) for t in range(fanout))
    if deg <= fanout:
        return list(range(deg))
    picked = []
    for t in range(fanout):
        j = deg - fanout + t
        p = mulhi(r[t], j + 1)
        picked.append(j if p in picked else p)
    return sorted(picked)


def sample(indptr, indices, data, seeds, fanout, replace, rng_seed, rng_ctr=0):
    """(offsets, nbr, eid) of DGLMISampleNeighbors; a seed outside the CSR has degree 0."""
    indptr = np.asarray(indptr, np.int64)
    n = len(indptr) - 1
    r = draws(rng_seed, rng_ctr, np.arange(len(seeds)), fanout)
    offsets, nbr, eid = [0], [], []
    for i, s in enumerate(seeds):
        start, deg = (int(indptr[s]), int(indptr[s + 1] - indptr[s])) if 0 <= s < n else (0, 0)
        for p in pick_positions(r[i], deg, fanout, replace):
            nbr.append(indices[start + p])
            eid.append(data[start + p])
        offsets.append(len(nbr))
    return (np.asarray(offsets, np.int64), np.asarray(nbr, np.int32), np.asarray(eid, np.int64))


def gather_rows(indptr, indices, data, rows):
    indptr = np.asarray(indptr, np.int64)
    sl = [slice(int(indptr[r]), int(indptr[r + 1])) for r in rows]
    offsets = np.concatenate([[0], np.cumsum([s.stop - s.start for s in sl])]).astype(np.int64)
    cat = lambda a, dt: (np.concatenate([np.asarray(a)[s] for s in sl]) if sl else
                         np.empty(0)).astype(dt)
    return offsets, cat(indices, np.int32), cat(data, np.int64)


def relabel(dst_nodes, src, include_dst=True):
    """(src_nodes, new_src, owners among the destinations) of DGLMIBlockRelabel*."""
    first = {}
    seq = (list(dst_nodes) if include_dst else []) + list(src)
    for v in seq:
        if v not in first:
            first[v] = len(first)
    uniq = len(set(dst_nodes)) if include_dst else 0
    src_nodes = np.asarray(sorted(first, key=first.get), np.int64)
    return src_nodes, np.asarray([first[v] for v in src], np.int32), uniq
