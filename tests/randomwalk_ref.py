"""Numpy restatement of the random-walk and visit-count contracts of include/dglmi.h
(DGLMIRandomWalk, DGLMIVisitTopK), written from the header text, not from the kernels.  Shared
by test_randomwalk_cpu.py, test_randomwalk_gpu.py, test_visit_topk_gpu.py and
test_pinsage_gpu.py.  The Philox is sampling_ref.py's."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sampling_ref import MASK, S32, philox4x32_10  # noqa: E402


def threshold(p):
    """restart[t] of a stopping probability p (a double): min(2^32, floor(p 2^32))."""
    return min(2 ** 32, int(math.floor(float(p) * 2.0 ** 32))) if p < 1 else 2 ** 32


def walk_draws(rng_seed, rng_ctr, num_walks, L):
    """(x, y) of every walk i < num_walks and step t < L: two (num_walks, L) uint64 arrays."""
    i = np.arange(num_walks, dtype=np.uint64).reshape(-1, 1)
    t = np.arange(max(L, 1), dtype=np.uint64).reshape(1, -1)
    c = np.broadcast_to(np.uint64(rng_ctr) + t, (num_walks, t.shape[1]))  # mod 2^64 by wrap
    s = np.broadcast_to(i, c.shape)
    seed = np.uint64(rng_seed)
    x, y, _, _ = philox4x32_10(c & MASK, c >> S32, s & MASK, s >> S32, seed & MASK, seed >> S32)
    return x[:, :L], y[:, :L]


def walk(csrs, metapath, seeds, restart, rng_seed, rng_ctr=0):
    """traces (len(seeds), L + 1) int64.  ``csrs``: a list of (indptr, indices) host arrays;
    ``metapath``: L indices into it; ``restart``: L thresholds or None."""
    L = len(metapath)
    n = len(seeds)
    x, y = walk_draws(rng_seed, rng_ctr, n, L)
    traces = np.full((n, L + 1), -1, np.int64)
    for i in range(n):
        v = int(seeds[i])
        traces[i, 0] = v
        for t in range(L):
            rel = int(metapath[t])
            deg = 0
            if 0 <= rel < len(csrs):
                indptr, indices = csrs[rel]
                if 0 <= v < len(indptr) - 1:
                    start = int(indptr[v])
                    deg = int(indptr[v + 1]) - start
            if deg == 0:
                break
            v = int(indices[start + ((int(x[i, t]) * deg) >> 32)])
            traces[i, t + 1] = v
            if restart is not None and int(y[i, t]) < int(restart[t]):
                break
    return traces


def visit_topk(traces, walks_per_seed, col0, col_step, k):
    """(nbr (S, k) int32, cnt (S, k) int32, num (S) int32) of DGLMIVisitTopK."""
    traces = np.asarray(traces, np.int64)
    S = traces.shape[0] // walks_per_seed
    nbr = np.full((S, k), -1, np.int32)
    cnt = np.zeros((S, k), np.int32)
    num = np.zeros(S, np.int32)
    for s in range(S):
        cand = traces[s * walks_per_seed:(s + 1) * walks_per_seed, col0::col_step].reshape(-1)
        cand = cand[(cand >= 0) & (cand < 2 ** 31 - 1)]
        ids, counts = np.unique(cand, return_counts=True)
        order = sorted(range(len(ids)), key=lambda j: (-int(counts[j]), int(ids[j])))[:k]
        num[s] = len(order)
        nbr[s, :len(order)] = ids[order]
        cnt[s, :len(order)] = counts[order]
    return nbr, cnt, num


def pinsage(csrs, metapath, hops, seeds, num_walks, restart, k, rng_seed, rng_ctr=0):
    """(src, dst, weights) of the samplers: the walks of every seed slot, their counts at the
    columns hops, 2 hops, .., the padded rows compacted seed by seed."""
    rep = np.repeat(np.asarray(seeds, np.int64), num_walks)
    traces = walk(csrs, metapath, rep, restart, rng_seed, rng_ctr)
    nbr, cnt, num = visit_topk(traces, num_walks, hops, hops, k)
    src, dst, w = [], [], []
    for s, seed in enumerate(seeds):
        src.extend(nbr[s, :num[s]])
        dst.extend([seed] * int(num[s]))
        w.extend(cnt[s, :num[s]])
    return np.asarray(src, np.int64), np.asarray(dst, np.int64), np.asarray(w, np.int64)
