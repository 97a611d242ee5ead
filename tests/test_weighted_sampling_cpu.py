"""Weighted neighbour sampling and select_topk without a GPU: the names, every host-side
validation error (raised before any launch, so host graphs reach them), and the contract's
arithmetic and distributions, checked on the restatement (``weighted_sampling_ref.py``) alone.

Distributions.  Pearson's statistic against the exact probabilities is compared with the
1 - 1e-6 quantile of chi-square, computed as ``test_sampling_cpu.py`` computes it.  Without
replacement the outcome of a slot is its (unordered) set of picks, whose exact probability is
the sum over both orders of successive sampling; slots are independent, so the statistic is
chi-square with (outcomes - 1) degrees of freedom.  With replacement the counts of the
positions are multinomial over slots x fanout independent draws.  In the 50-bin test without
replacement a slot's picks are negatively correlated, which makes the statistic smaller, as
in the uniform test; there the weights are equal inside a bin and differ between bins by at
most 2 : 1 with fanout / degree = 0.002, so first-order inclusion probabilities
(fanout w / sum w) are exact to about that ratio, far inside the quantile's margin."""
import itertools
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch as th

import dgl
from dgl import kernel as K

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_ref as R  # noqa: E402
import weighted_sampling_ref as W  # noqa: E402


def test_names_are_importable():
    from dgl.sampling import sample_neighbors, select_topk
    assert dgl.sampling.select_topk is select_topk
    assert dgl.sampling.sample_neighbors is sample_neighbors
    assert "select_topk" in dgl.sampling.__all__
    for name in ("sample_neighbors_weighted", "select_topk"):
        assert callable(getattr(K, name))
    from dgl import _ffi
    assert "DGLMISampleNeighborsWeighted" in _ffi.EXPORTED and "DGLMISelectTopk" in _ffi.EXPORTED


def _g(feat=True):
    g = dgl.DGLGraph()
    g.add_nodes(6)
    g.add_edges([0, 1, 2, 3, 4], [1, 2, 3, 4, 5])
    if feat:
        g.edata["p"] = th.tensor([1.0, 2.0, 3.0, 4.0, 5.0])
        g.edata["i"] = th.tensor([1, 2, 3, 4, 5])
        g.edata["wide"] = th.ones(5, 2)
    return g


@pytest.fixture
def no_launch(monkeypatch):
    """Fail the test if anything reaches the library's launching entries."""
    def boom(*a, **k):
        raise AssertionError("a launch was attempted before validation finished")
    for name in ("sample_neighbors", "sample_neighbors_weighted", "select_topk", "csr_gather_rows",
                 "block_relabel"):
        monkeypatch.setattr(K, name, boom)


def test_missing_feature(no_launch):
    with pytest.raises(dgl.DGLError, match="weighted sampling"):
        dgl.sampling.sample_neighbors(_g(), [1], 2, prob="nope")
    with pytest.raises(dgl.DGLError, match="edge feature 'nope'"):
        dgl.sampling.select_topk(_g(), 2, "nope")


@pytest.mark.parametrize("prob", ["i", th.tensor([1, 2, 3, 4, 5]), th.ones(5, dtype=th.float16),
                                  th.ones(5, dtype=th.bool)])
def test_prob_must_be_float(no_launch, prob):
    with pytest.raises(dgl.DGLError, match="prob must be of dtype torch.float32 or torch.float64"):
        dgl.sampling.sample_neighbors(_g(), [1], 2, prob=prob)


def test_topk_weight_dtype(no_launch):
    with pytest.raises(dgl.DGLError, match="weight must be of dtype"):
        dgl.sampling.select_topk(_g(), 2, th.ones(5, dtype=th.float16))
    with pytest.raises(dgl.DGLError, match="weight must be of dtype"):
        dgl.sampling.select_topk(_g(), 2, th.ones(5, dtype=th.int16))


@pytest.mark.parametrize("prob", ["wide", th.ones(4), th.ones(6), th.ones(5, 2), th.ones(1, 5),
                                  th.ones(()), th.ones(5, 1, 1)])
def test_wrong_shape_or_length(no_launch, prob):
    with pytest.raises(dgl.DGLError, match=r"must have shape \(5,\) or \(5, 1\)"):
        dgl.sampling.sample_neighbors(_g(), [1], 2, prob=prob)
    with pytest.raises(dgl.DGLError, match=r"must have shape \(5,\) or \(5, 1\)"):
        dgl.sampling.select_topk(_g(), 2, prob)


@pytest.mark.parametrize("prob", [[1.0] * 5, np.ones(5), 3.0])
def test_prob_must_be_a_name_or_a_tensor(no_launch, prob):
    with pytest.raises(dgl.DGLError, match="an edge feature name or a tensor"):
        dgl.sampling.sample_neighbors(_g(), [1], 2, prob=prob)
    with pytest.raises(dgl.DGLError, match="an edge feature name or a tensor"):
        dgl.sampling.select_topk(_g(), 2, prob)


def test_wrong_device(no_launch, monkeypatch):
    """The graph lives on cuda:0 (a device-built graph records its device); weights on any
    device but that one and the host are refused before the ids are touched."""
    from dgl.sampling import neighbor as N
    monkeypatch.setattr(N, "_built_on", lambda index: th.device("cuda", 0))
    w = th.ones(5, device="meta")
    with pytest.raises(dgl.DGLError, match="prob is on meta, the graph on cuda:0"):
        dgl.sampling.sample_neighbors(_g(), [1], 2, prob=w)
    with pytest.raises(dgl.DGLError, match="weight is on meta, the graph on cuda:0"):
        dgl.sampling.select_topk(_g(), 2, w)


def test_limits(no_launch):
    top = K.sample_max_fanout()
    with pytest.raises(dgl.DGLError, match="fanout = %d is above the kernel's limit of %d"
                       % (top + 1, top)):
        dgl.sampling.sample_neighbors(_g(), [1], top + 1, prob="p")
    with pytest.raises(dgl.DGLError, match="fanout must not be negative"):
        dgl.sampling.sample_neighbors(_g(), [1], -1, prob="p")
    with pytest.raises(dgl.DGLError, match="k = %d is above the kernel's limit of %d"
                       % (top + 1, top)):
        dgl.sampling.select_topk(_g(), top + 1, "p")
    with pytest.raises(dgl.DGLError, match="k must not be negative"):
        dgl.sampling.select_topk(_g(), -2, "p")


@pytest.mark.parametrize("k", [2.0, "3", None, True])
def test_k_must_be_an_int(no_launch, k):
    with pytest.raises(dgl.DGLError, match="k must be an int"):
        dgl.sampling.select_topk(_g(), k, "p")


@pytest.mark.parametrize("edge_dir", ["both", "IN", None, 0])
def test_bad_edge_dir(no_launch, edge_dir):
    with pytest.raises(dgl.DGLError, match="edge_dir must be 'in' or 'out'"):
        dgl.sampling.select_topk(_g(), 2, "p", edge_dir=edge_dir)
    with pytest.raises(dgl.DGLError, match="edge_dir must be 'in' or 'out'"):
        dgl.sampling.sample_neighbors(_g(), [1], 2, edge_dir=edge_dir, prob="p")


def test_topk_nodes_and_graph_errors(no_launch, monkeypatch):
    with pytest.raises(dgl.DGLError, match="out of range"):
        dgl.sampling.select_topk(_g(), 2, "p", nodes=[6])
    g = dgl.heterograph({("a", "x", "b"): ([0], [0]), ("b", "y", "a"): ([0], [0])})
    with pytest.raises(dgl.DGLError, match="more than one edge type"):
        dgl.sampling.select_topk(g, 2, "p")
    monkeypatch.setattr(th.cuda, "is_available", lambda: False)
    with pytest.raises(dgl.DGLError, match="ROCm devices only"):
        dgl.sampling.select_topk(_g(), 2, "p")
    with pytest.raises(dgl.DGLError, match="ROCm devices only"):
        dgl.sampling.sample_neighbors(_g(), [1], 2, prob="p")


def test_random_walk_prob_still_raises():
    g = dgl.graph(([0, 1], [1, 0]))
    with pytest.raises(dgl.DGLError):
        dgl.sampling.random_walk(g, [0], length=2, prob="p")


# ---- the restatement itself ----------------------------------------------------------
def test_exp_key_against_log2():
    """|E / 2^40 - exact| <= 2^-38 at the extreme draws and 2,000 random ones; E > 0."""
    rng = np.random.default_rng(20261021)
    rs = [0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1] + \
        [int(v) for v in rng.integers(0, 2 ** 32, 2000)]
    worst = 0.0
    for r in rs:
        E = W.exp_key(r)
        assert 0 < E < 2 ** 46
        exact = 33.0 - math.log2(2 * r + 1)  # -log2((r + 1/2) / 2^32)
        worst = max(worst, abs(E / 2.0 ** 40 - exact))
    print("worst |E / 2^40 - exact| = %.3g" % worst)
    assert worst <= 2.0 ** -38
    assert W.exp_key(2 ** 32 - 1) >= 185
    assert W.exp_key(0) == 33 << 40
    assert W.exp_keys(rs).tolist() == [W.exp_key(r) for r in rs]  # the array form


def test_draw_layouts():
    seed, ctr, slot = 0x1234567890ABCDEF, 2 ** 64 - 1, 2 ** 33 + 1
    for p in (0, 3, 4, 5, 2 ** 34 + 2):
        c = (ctr + (p >> 2)) % 2 ** 64
        blk = R.philox4x32_10(c & 0xFFFFFFFF, c >> 32, slot & 0xFFFFFFFF, slot >> 32,
                              0x90ABCDEF, 0x12345678)
        assert W.draws_at(seed, ctr, slot, [p]).tolist() == [int(blk[p & 3])]
    for t in range(6):
        c = (ctr + (t >> 1)) % 2 ** 64
        blk = [int(v) for v in R.philox4x32_10(c & 0xFFFFFFFF, c >> 32, slot & 0xFFFFFFFF,
                                               slot >> 32, 0x90ABCDEF, 0x12345678)]
        lo, hi = (blk[2], blk[3]) if t & 1 else (blk[0], blk[1])
        assert W.draw64(seed, ctr, slot, t) == hi * 2 ** 32 + lo
    # positions below 2^32 take the uniform sampler's draws
    assert W.draws_at(seed, 5, 7, range(9)).tolist() == R.draws(seed, 5, [7], 9)[0].tolist()


def test_eligibility():
    f32, f64 = np.float32, np.float64
    for w in (f32(1), f32(1e-45), f32(3.4e38), f64(2.0 ** -900), f64(1e308)):
        assert W.eligible(w)
    for w in (f32(0), f32(-0.0), f32(-1), f32("nan"), f32("inf"), f32("-inf"), f64(0),
              f64(2.0 ** -901), f64(5e-324), f64("nan"), f64("inf"), f64(-2.0)):
        assert not W.eligible(w)


def test_quantisation_is_exact():
    ws = np.array([1.0, 3.0, 0.75, 2.0 ** -29, 2.0 ** -30, 3 * 2.0 ** -31, 0.0, np.nan])
    # max = 3 = 0.75 * 2^2: e = 2, q = floor(w * 2^29)
    assert W.quantised_exact(ws) == [2 ** 29, 3 * 2 ** 29, 3 * 2 ** 27, 1, 0, 0, 0, 0]
    q = W.quantised_exact(np.array([5.0, 1e-3], np.float32))
    assert 2 ** 30 <= q[0] < 2 ** 31
    assert q[1] == int(Fraction(float(np.float32(1e-3))) * Fraction(2) ** 28)
    rng = np.random.default_rng(3)
    for dt, lo in ((np.float32, -149), (np.float64, -1000)):  # the array form, any exponent
        w = np.ldexp(rng.uniform(0.5, 1, 200), rng.integers(lo, 100, 200)).astype(dt)
        w[::7] = 0
        for part in (w, w[:20], w[w < 1e-30]):
            assert W.quantised(part).tolist() == W.quantised_exact(part)


def test_count_rules():
    w = np.array([1, 0, 2, np.nan, 3, -1, np.inf, 4], np.float32)  # row 3: nz = 4 of 8
    indptr = [0, 0, 1, 2, 10]
    data = [1, 0, 0, 1, 2, 3, 4, 5, 6, 7]  # row 1: weight 0; row 2: weight 1
    indices = np.arange(10) * 2
    seeds = [3, 0, 1, 2, 3, 9]
    for fanout, want in ((2, [2, 0, 0, 1, 2, 0]), (4, [4, 0, 0, 1, 4, 0]), (6, [4, 0, 0, 1, 4, 0]),
                         (0, [0] * 6)):
        off, nbr, eid = W.sample_weighted(indptr, indices, data, seeds, fanout, False, w, 1)
        assert np.diff(off).tolist() == want
        assert np.all(np.isin(eid[:off[1]], [0, 2, 4, 7]))
        for a, b in zip(off[:-1], off[1:]):
            assert np.all(np.diff(nbr[a:b]) > 0)  # ascending position, no repeats
    off, nbr, eid = W.sample_weighted(indptr, indices, data, seeds, 6, False, w, 1)
    assert eid[:4].tolist() == [0, 2, 4, 7]  # nz < fanout < deg: the eligible entries
    for fanout, want in ((3, [3, 0, 0, 3, 3, 0]), (0, [0] * 6)):
        off, nbr, eid = W.sample_weighted(indptr, indices, data, seeds, fanout, True, w, 1)
        assert np.diff(off).tolist() == want
        assert np.all(np.isin(eid, [0, 2, 4, 7]))
        for a, b in zip(off[:-1], off[1:]):
            assert np.all(np.diff(nbr[a:b]) >= 0)
    off, nbr, eid = W.select_topk(indptr, indices, data, seeds, 3, w)
    assert np.diff(off).tolist() == [3, 0, 1, 1, 3, 0]  # min(deg, k): the degree rule
    assert eid[:3].tolist() == [6, 7, 4]  # inf, 4, 3
    off, nbr, eid = W.select_topk(indptr, indices, data, seeds, 8, w, ascending=True)
    assert eid[:8].tolist() == [5, 1, 0, 2, 4, 7, 6, 3]  # -1 0 1 2 3 4 inf nan


def test_topk_order_rules():
    w = np.array([0.0, -0.0, np.nan, 1.0, -np.inf, 1.0, np.inf])
    assert W.topk_positions(list(w), 7, False) == [6, 3, 5, 0, 1, 4, 2]
    assert W.topk_positions(list(w), 7, True) == [4, 0, 1, 3, 5, 6, 2]
    assert W.topk_positions([7] * 5, 3, False) == [0, 1, 2]
    big = np.array([2 ** 63 - 1, -2 ** 63, 0, 2 ** 63 - 2], np.int64)
    assert W.topk_positions(list(big), 4, False) == [0, 3, 2, 1]
    assert W.topk_positions(list(big), 4, True) == [1, 2, 3, 0]


def _chi2_quantile(df, tail=1e-6):
    try:
        from scipy import stats
        return float(stats.chi2.isf(tail, df))
    except ImportError:  # Wilson-Hilferty: chi2_df ~ df (1 - 2/(9 df) + z sqrt(2/(9 df)))^3
        z = 4.753424308822899  # the 1 - 1e-6 quantile of the standard normal
        a = 2.0 / (9.0 * df)
        return df * (1.0 - a + z * a ** 0.5) ** 3


WEIGHTS = np.array([1, 2, 3, 4, 0, 6], np.float32)


@pytest.mark.parametrize("seed", [12345])
def test_pairs_without_replacement(seed):
    """Fan-out 2 of (1, 2, 3, 4, 0, 6): the ten pairs of successive sampling, 9 degrees of
    freedom.  (Measured when the contract was written: 11.4 with seed 12345.)"""
    slots = 20000
    w = [Fraction(int(v)) for v in WEIGHTS]
    tot = sum(w)
    el = [p for p in range(6) if w[p] > 0]
    prob = {(a, b): float(w[a] / tot * w[b] / (tot - w[a]) + w[b] / tot * w[a] / (tot - w[b]))
            for a, b in itertools.combinations(el, 2)}
    assert len(prob) == 10 and abs(sum(prob.values()) - 1) < 1e-12
    count = dict.fromkeys(prob, 0)
    for i in range(slots):
        picks = W.weighted_positions(list(WEIGHTS), 2, False, seed, 0, i)
        assert len(picks) == 2 and picks[0] < picks[1] and 4 not in picks
        count[tuple(picks)] += 1
    stat = sum((count[k] - slots * prob[k]) ** 2 / (slots * prob[k]) for k in prob)
    bound = _chi2_quantile(9)
    print("chi2 pairs seed=%d: %.2f (bound %.2f)" % (seed, stat, bound))
    assert stat < bound


@pytest.mark.parametrize("seed", [777])
def test_counts_with_replacement(seed):
    """Fan-out 4 of the same weights: five positions of probability w / 16, 4 degrees of
    freedom.  (Measured when the contract was written: 3.4 with seed 777.)"""
    slots = 20000
    count = np.zeros(6, np.int64)
    for i in range(slots):
        picks = W.weighted_positions(list(WEIGHTS), 4, True, seed, 0, i)
        assert len(picks) == 4 and picks == sorted(picks)
        np.add.at(count, picks, 1)
    assert count[4] == 0
    expect = slots * 4 * WEIGHTS.astype(np.float64) / 16.0
    keep = expect > 0
    stat = float(((count[keep] - expect[keep]) ** 2 / expect[keep]).sum())
    bound = _chi2_quantile(4)
    print("chi2 replace seed=%d: %.2f (bound %.2f)" % (seed, stat, bound))
    assert stat < bound


@pytest.mark.parametrize("replace", [True, False])
def test_hub_row_in_bins(replace):
    """A degree-5,000 row in 50 bins of 100 equal weights, bin b of weight 1 + b / 49; every
    tenth entry has weight 0 and is never drawn."""
    deg, bins, fanout, slots, seed = 5000, 50, 10, 1500, 20261021
    w = np.repeat(1.0 + np.arange(bins) / (bins - 1.0), deg // bins).astype(np.float32)
    w[::10] = 0
    count = np.zeros(bins, np.int64)
    for i in range(slots):
        picks = W.weighted_positions(list(w), fanout, replace, seed, 0, i)
        assert len(picks) == fanout and all(w[p] > 0 for p in picks)
        if not replace:
            assert len(set(picks)) == fanout
        np.add.at(count, np.asarray(picks) // (deg // bins), 1)
    mass = w.astype(np.float64).reshape(bins, -1).sum(1)
    expect = slots * fanout * mass / mass.sum()
    stat = float(((count - expect) ** 2 / expect).sum())
    bound = _chi2_quantile(bins - 1)
    print("chi2 hub replace=%s: %.2f (bound %.2f)" % (replace, stat, bound))
    assert stat < bound
