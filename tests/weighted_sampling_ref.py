"""Numpy and Python-int restatement of DGLMISampleNeighborsWeighted and DGLMISelectTopk of
include/dglmi.h, written from the header text, not from the kernels.  ``exp_key`` and
``quantised_exact`` are the header's words in Python ints and rationals; ``exp_keys`` and
``quantised`` are their array forms, which test_weighted_sampling_cpu.py holds against them.
The one float operation is numpy's fp64 division.  Shared by test_weighted_sampling_cpu.py
and test_weighted_sampling_gpu.py."""
import math
from fractions import Fraction

import numpy as np

import sampling_ref as R

MASK64 = (1 << 64) - 1
U = np.uint64


def exp_key(r):
    """E(r): -log2((r + 1/2) / 2^32) in 40 fractional bits (Python ints)."""
    y = 2 * int(r) + 1
    n = y.bit_length() - 1
    m = y << (63 - n)
    bits = 0
    for _ in range(40):
        sq = (m * m) >> 63
        if sq >= 1 << 64:
            bits, m = 2 * bits + 1, sq >> 1
        else:
            bits, m = 2 * bits, sq
    return (33 << 40) - ((n << 40) + bits)


def exp_keys(r):
    """``exp_key`` for an array of draws: the 128-bit square in 32-bit limbs of uint64."""
    y = U(2) * np.asarray(r, U) + U(1)
    n = (np.frexp(y.astype(np.float64))[1] - 1).astype(U)  # y < 2^34 is exact in fp64
    m = y << (U(63) - n)
    bits = np.zeros_like(m)
    lo31 = U(2 ** 31 - 1)
    with np.errstate(over="ignore"):
        for _ in range(40):
            a, b = m >> U(32), m & R.MASK
            aa, ab, bb = a * a, a * b, b * b  # m m = aa 2^64 + ab 2^33 + bb
            lo = bb + ((ab & lo31) << U(33))
            hi = aa + (ab >> U(31)) + (lo < bb).astype(U)
            one = hi >> U(63)
            m = np.where(one == 1, hi, (hi << U(1)) | (lo >> U(63)))
            bits = (bits << U(1)) | one
    return (U(33) << U(40)) - ((n << U(40)) + bits)


def eligible(ws):
    """Finite and greater than 0; a float64 also at least 2^-900.  An array of bool."""
    ws = np.asarray(ws)
    assert ws.dtype in (np.float32, np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(ws) & (ws > 0)
        if ws.dtype == np.float64:
            ok &= ws >= 2.0 ** -900
    return ok


def _blocks(rng_seed, ctr, slot):
    ctr = np.asarray(ctr, U)
    slot = np.full(ctr.shape, slot, U)
    seed = int(rng_seed) & MASK64
    return R.philox4x32_10(ctr & R.MASK, ctr >> R.S32, slot & R.MASK, slot >> R.S32,
                           seed & 0xFFFFFFFF, seed >> 32)


def draws_at(rng_seed, rng_ctr, slot, positions):
    """r(i, p) for 64-bit positions p: component p & 3 of the block at rng_ctr + (p >> 2)."""
    p = np.asarray(list(positions), U).reshape(-1)
    with np.errstate(over="ignore"):
        blk = _blocks(rng_seed, U(int(rng_ctr) & MASK64) + (p >> U(2)), slot)
    return np.choose((p & U(3)).astype(np.int64), blk) if p.size else np.zeros(0, U)


def draw64(rng_seed, rng_ctr, slot, t):
    """R_t: (lo, hi) = words (x, y) for even t, (z, w) for odd t at counter rng_ctr + (t >> 1)."""
    blk = _blocks(rng_seed, [(int(rng_ctr) + (t >> 1)) & MASK64], slot)
    lo, hi = (int(blk[2][0]), int(blk[3][0])) if t & 1 else (int(blk[0][0]), int(blk[1][0]))
    return (hi << 32) | lo


def key_bits(E, w):
    """The bits of the fp64 quotients double(E) / double(w) as uint64."""
    q = np.asarray(E).astype(np.float64) / np.asarray(w).astype(np.float64)
    return q.view(U)


def quantised_exact(ws):
    """q_p = floor(w_p 2^(31 - e)), e the binary exponent of the largest eligible weight, in
    rationals."""
    ok = eligible(ws)
    if not ok.any():
        return [0] * len(ws)
    e = math.frexp(max(float(w) for w in np.asarray(ws)[ok]))[1]
    scale = Fraction(2) ** (31 - e)
    return [int(Fraction(float(w)) * scale) if o else 0 for w, o in zip(ws, ok)]


def quantised(ws):
    """``quantised_exact`` as int64: ldexp scales by a power of two exactly, and where it
    underflows the product is below 1 and its floor 0 either way."""
    ws = np.asarray(ws)
    ok = eligible(ws)
    if not ok.any():
        return np.zeros(len(ws), np.int64)
    w = np.where(ok, ws, 0).astype(np.float64)
    e = math.frexp(float(w.max()))[1]
    return np.floor(np.ldexp(w, 31 - e)).astype(np.int64)


def weighted_positions(ws, fanout, replace, rng_seed, rng_ctr, slot):
    """The picks (ascending positions) of one seed slot whose row has the weights ``ws``."""
    ws = np.asarray(ws)
    el = np.flatnonzero(eligible(ws)) if len(ws) else np.zeros(0, np.int64)
    if not len(el) or fanout == 0:
        return []
    if replace:
        run = np.cumsum(quantised(ws))
        total = int(run[-1])
        picks = []
        for t in range(fanout):
            T = (draw64(rng_seed, rng_ctr, slot, t) * total) >> 64
            picks.append(int(np.searchsorted(run, T, side="right")))  # the first run > T
        return sorted(picks)
    if len(el) <= fanout:
        return [int(p) for p in el]
    keys = key_bits(exp_keys(draws_at(rng_seed, rng_ctr, slot, el)), ws[el])
    first = np.lexsort((el, keys))[:fanout]  # by key, then by position
    return sorted(int(p) for p in el[first])


def _rows(indptr, seeds):
    indptr = np.asarray(indptr, np.int64)
    n = len(indptr) - 1
    for i, s in enumerate(seeds):
        s = int(s)
        yield i, ((int(indptr[s]), int(indptr[s + 1] - indptr[s])) if 0 <= s < n else (0, 0))


def _emit(indices, data, per_seed):
    offsets, nbr, eid = [0], [], []
    for start, picks in per_seed:
        nbr += [indices[start + p] for p in picks]
        eid += [data[start + p] for p in picks]
        offsets.append(len(nbr))
    return (np.asarray(offsets, np.int64), np.asarray(nbr, np.int32), np.asarray(eid, np.int64))


def sample_weighted(indptr, indices, data, seeds, fanout, replace, weight, rng_seed, rng_ctr=0):
    """(offsets, nbr, eid) of DGLMISampleNeighborsWeighted; ``weight`` is indexed by edge id."""
    weight, data = np.asarray(weight), np.asarray(data, np.int64)
    out = []
    for i, (start, deg) in _rows(indptr, seeds):
        ws = weight[data[start:start + deg]]
        out.append((start, weighted_positions(ws, fanout, replace, rng_seed, rng_ctr, i)))
    return _emit(indices, data, out)


def topk_positions(ws, k, ascending):
    """The first k positions in (weight in the asked direction, position); -0.0 is +0.0 and a
    NaN ranks after every number in both directions."""
    def rank(p):
        w = ws[p]
        if isinstance(w, (float, np.floating)):
            if math.isnan(w):
                return (1, 0, p)
            w = float(w) + 0.0  # -0.0 + 0.0 is +0.0
        else:
            w = int(w)
        return (0, w if ascending else -w, p)
    return sorted(range(len(ws)), key=rank)[:k]


def select_topk(indptr, indices, data, seeds, k, weight, ascending=False):
    """(offsets, nbr, eid) of DGLMISelectTopk."""
    weight, data = np.asarray(weight), np.asarray(data, np.int64)
    out = []
    for _, (start, deg) in _rows(indptr, seeds):
        ws = weight[data[start:start + deg]]
        out.append((start, topk_positions(list(ws), k, ascending)))
    return _emit(indices, data, out)
