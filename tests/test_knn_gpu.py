"""k-NN graphs on the device: ``dgl.kernel.knn_select`` bit for bit against a numpy
restatement on exactly representable inputs, within the derived fp32 bound on continuous
ones, and the graphs / modules built on it.

Exact inputs: coordinates are multiples of 1/16 in [-2, 2) and D <= 256, so every
difference, square and partial sum is an fp32 number: every summation order gives the same
distance, ties are exact and frequent, and the strict total order (distance, NaN last,
then row id) fixes every entry of the result.

Continuous inputs: d = sum of D non-negative terms, each with a rounded subtraction and a
rounded square, summed by D - 1 rounded adds: relative error at most gamma_(D+2) =
(D+2) u / (1 - (D+2) u), u = 2^-24.  Comparisons between two such distances use
eps = 4 (D+2) 2^-24 (twice 2 gamma_(D+2))."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as th

import dgl
from dgl import kernel as K
from dgl.nn.pytorch import EdgeConv, KNNGraph, MaxPooling, SegmentedKNNGraph

pytestmark = pytest.mark.gpu
DEV = th.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def grid_points(rng, n, D):
    return (rng.integers(-32, 32, (n, D)) / 16.0).astype(np.float32)


def offsets_of(segs):
    off = np.zeros(len(segs) + 1, np.int64)
    np.cumsum(np.asarray(segs, np.int64), out=off[1:])
    return off


def dist32(a):
    """(m, m) fp32 distances of one point set: per feature, in ascending order, a rounded
    subtraction, a rounded square, a rounded add."""
    d = np.zeros((a.shape[0], a.shape[0]), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(a.shape[1]):
            t = a[:, None, f] - a[None, :, f]
            d = d + t * t
    return d


def ref_select(x, segs, k):
    """The contract in numpy: per segment, the k first candidates of every row under
    (distance ascending, NaN last, row id ascending); -1 / +inf past a short segment."""
    n = x.shape[0]
    nbr = np.full((n, k), -1, np.int32)
    dist = np.full((n, k), np.inf, np.float32)
    off = offsets_of(segs)
    for b in range(len(segs)):
        lo, hi = int(off[b]), int(off[b + 1])
        m = hi - lo
        if m == 0:
            continue
        d = dist32(x[lo:hi])
        ids = np.broadcast_to(np.arange(m), (m, m))
        order = np.lexsort((ids, d, np.isnan(d)), axis=-1)[:, :min(k, m)]
        nbr[lo:hi, :order.shape[1]] = order + lo
        dist[lo:hi, :order.shape[1]] = np.take_along_axis(d, order, 1)
    return nbr, dist


def run_select(x, segs, k):
    xt = th.from_numpy(x).to(DEV)
    off = th.from_numpy(offsets_of(segs)).to(DEV)
    nbr, dist = K.knn_select(xt, off, k, want_dist=True)
    nbr2, dist2 = K.knn_select(xt, off, k, want_dist=True)
    only = K.knn_select(xt, off, k)
    assert th.equal(nbr, nbr2) and th.equal(dist.view(th.int32), dist2.view(th.int32))
    assert th.equal(nbr, only)
    assert nbr.dtype == th.int32 and dist.dtype == th.float32
    return nbr.cpu().numpy(), dist.cpu().numpy()


def check_exact(x, segs, k):
    nbr, dist = run_select(x, segs, k)
    r_nbr, r_dist = ref_select(x, segs, k)
    np.testing.assert_array_equal(nbr, r_nbr)
    nan = np.isnan(r_dist)
    np.testing.assert_array_equal(np.isnan(dist), nan)
    np.testing.assert_array_equal(np.where(nan, 0, dist).view(np.uint32),
                                  np.where(nan, 0, r_dist).view(np.uint32))
    return nbr, dist


def tile(D, k):
    return K.knn_tile(D, k)


# ---- exact: segment shapes ----------------------------------------------------------------
SEG_CASES = {
    "lengths": lambda k, TQ, TC: [k, k + 1, TQ - 1, TQ, TQ + 1, TC + 1, 2 * TC + 3],
    "boundary_in_tile": lambda k, TQ, TC: [TQ // 2 + 3, TQ, TQ // 2 - 1],
    "tile_of_length_k": lambda k, TQ, TC: [k] * (2 * (TQ // k) + 3),
    "empty_segments": lambda k, TQ, TC: [0, 0, 7, 0, TQ + 5, 0, 0, 9, 0, 0],
    "one_segment": lambda k, TQ, TC: [3 * TQ + 5],
    "one_row_tail": lambda k, TQ, TC: [2 * TQ, 1 + k],
}


@pytest.mark.parametrize("case", sorted(SEG_CASES))
def test_exact_segment_shapes(case):
    D, k = 3, 4
    TQ, TC, _ = tile(D, k)
    segs = SEG_CASES[case](k, TQ, TC)
    x = grid_points(np.random.default_rng(1), sum(segs), D)
    check_exact(x, segs, k)


@pytest.mark.parametrize("d", ["1", "2", "3", "4", "5", "DC-1", "DC", "DC+1", "2*DC+3", "256"])
def test_exact_feature_lengths(d):
    k = 5
    DC = tile(3, k)[2]
    D = eval(d, {"DC": DC})
    TQ, TC, _ = tile(D, k)
    segs = [TQ + 9, 13, TC + 1]
    x = grid_points(np.random.default_rng(2), sum(segs), D)
    check_exact(x, segs, k)


@pytest.mark.parametrize("kk", ["1", "2", "20", "32", "33", "MaxK"])
@pytest.mark.parametrize("D", [3, 35])
def test_exact_k(kk, D):
    MaxK = K.knn_max_k()
    k = eval(kk, {"MaxK": MaxK})
    TQ, TC, _ = tile(D, k)
    segs = [k, k + 1, MaxK, MaxK + 1, 2 * TC + 3]
    x = grid_points(np.random.default_rng(3), sum(segs), D)
    check_exact(x, segs, k)


# ---- exact: adversarial candidate orders ------------------------------------------------------
def line(m, far_to_near):
    """m points on a line, coordinates non-increasing (far to near, seen from the last
    point: every tile brings closer candidates) or non-decreasing in the index."""
    c = (np.arange(m) * 64 // m).astype(np.float32) / 16.0 - 2.0
    if far_to_near:
        c = c[::-1].copy()
    return np.stack([c, np.zeros_like(c)], 1)


@pytest.mark.parametrize("far_to_near", [True, False])
@pytest.mark.parametrize("k", [4, 33])
def test_exact_line(far_to_near, k):
    TQ, TC, _ = tile(2, k)
    m = 3 * TC + 7
    x = np.concatenate([line(m, far_to_near), line(TQ - 3, far_to_near)])
    check_exact(x, [m, TQ - 3], k)


def test_exact_all_identical():
    k = 5
    TQ, _, _ = tile(3, k)
    segs = [TQ + 7, 9]
    x = np.full((sum(segs), 3), 0.5, np.float32)
    nbr, dist = check_exact(x, segs, k)
    # the lowest k ids of the segment, which need not contain the row itself
    np.testing.assert_array_equal(nbr[:segs[0]], np.broadcast_to(np.arange(k), (segs[0], k)))
    np.testing.assert_array_equal(nbr[segs[0]:], np.broadcast_to(segs[0] + np.arange(k), (9, k)))
    assert (dist == 0).all()


def test_exact_duplicated_pairs():
    k = 6
    TQ, TC, _ = tile(3, k)
    segs = [TQ + 6, 2 * TC + 2]
    x = grid_points(np.random.default_rng(4), sum(segs), 3)
    x[1::2] = x[0::2]
    nbr, dist = check_exact(x, segs, k)
    # a point and its copy come first, the lower id before the higher
    even = np.arange(0, sum(segs), 2)
    np.testing.assert_array_equal(nbr[even, 0], even)
    np.testing.assert_array_equal(nbr[even + 1, 0], even)
    assert (dist[:, :2] == 0).all()


# ---- exact: special values -----------------------------------------------------------------
def test_exact_nan_point():
    k = 6
    TQ, _, _ = tile(3, k)
    segs = [TQ + 1, k, 11]
    x = grid_points(np.random.default_rng(5), sum(segs), 3)
    p = segs[0] + 2
    x[p, 1] = np.nan
    nbr, dist = check_exact(x, segs, k)
    rows = np.arange(segs[0], segs[0] + k)
    others = rows[rows != p]
    assert (nbr[others, k - 1] == p).all() and np.isnan(dist[others, k - 1]).all()
    assert not np.isnan(dist[others, :k - 1]).any()
    np.testing.assert_array_equal(nbr[p], rows)  # all NaN: the segment's lowest k ids
    assert np.isnan(dist[p]).all()


def test_exact_inf_coordinate():
    k = 4
    TQ, _, _ = tile(3, k)
    segs = [TQ + 3, 8]
    x = grid_points(np.random.default_rng(6), sum(segs), 3)
    x[5, 0] = np.inf
    x[segs[0] + 1, 2] = -np.inf
    nbr, dist = check_exact(x, segs, k)
    assert np.isinf(dist[5][~np.isnan(dist[5])]).all()  # inf to the others, NaN to itself


def test_short_segment_tails():
    k = 5
    TQ, _, _ = tile(3, k)
    segs = [3, TQ, 0, 2, 1]
    x = grid_points(np.random.default_rng(7), sum(segs), 3)
    nbr, dist = check_exact(x, segs, k)
    assert (nbr[:3, 3:] == -1).all() and np.isposinf(dist[:3, 3:]).all()
    assert (nbr[:3, :3] >= 0).all()
    assert (nbr[-1] == [sum(segs) - 1, -1, -1, -1, -1]).all()
    assert (nbr[3:3 + TQ] >= 3).all() and (nbr[3:3 + TQ] < 3 + TQ).all()


def test_c_entry_limits():
    x = th.zeros(8, 3, device=DEV)
    off = th.tensor([0, 8], device=DEV)
    for k in (0, K.knn_max_k() + 1):
        with pytest.raises(dgl.DGLError, match="between 1 and %d" % K.knn_max_k()):
            K.knn_select(x, off, k)
    with pytest.raises(dgl.DGLError, match="2\\^31"):
        K.knn_select(th.empty(2 ** 25, 1, device=DEV), th.tensor([0, 2 ** 25], device=DEV), 64)
    assert K.knn_select(x[:0], th.tensor([0], device=DEV), 3).shape == (0, 3)


# ---- continuous inputs ----------------------------------------------------------------------
@pytest.mark.parametrize("D", [3, 64, 130])
def test_continuous(D):
    k = 20
    TQ, TC, _ = tile(D, k)
    segs = [TQ + 30, 2 * TC + 45, 77]
    n = sum(segs)
    x = np.random.default_rng(8).standard_normal((n, D)).astype(np.float32)
    nbr, dist = run_select(x, segs, k)
    u = 2.0 ** -24
    gamma = (D + 2) * u / (1 - (D + 2) * u)
    eps = 4 * (D + 2) * u
    off = offsets_of(segs)
    x64 = x.astype(np.float64)
    for b in range(len(segs)):
        lo, hi = int(off[b]), int(off[b + 1])
        a = x64[lo:hi]
        d64 = ((a[:, None, :] - a[None, :, :]) ** 2).sum(-1)
        got = nbr[lo:hi].astype(np.int64)
        assert (got >= lo).all() and (got < hi).all()
        s = np.sort(got, 1)
        assert (s[:, 1:] != s[:, :-1]).all()
        dg = np.take_along_axis(d64, got - lo, 1)
        kth = np.sort(d64, 1)[:, k - 1:k]
        assert (dg <= kth * (1 + eps)).all()
        assert (dg[:, :-1] <= dg[:, 1:] * (1 + eps)).all()
        assert (np.abs(dist[lo:hi].astype(np.float64) - dg) <= gamma * dg).all()
        assert (got[:, 0] == np.arange(lo, hi)).all() and (dist[lo:hi, 0] == 0).all()


# ---- graph level ----------------------------------------------------------------------------
def ref_edges(x, segs, k):
    """The reference's edges and edge ids: csr_matrix((1, (neighbour, point))).tocoo() --
    ascending (neighbour, point)."""
    nbr, _ = ref_select(x, segs, k)
    src = nbr.reshape(-1).astype(np.int64)
    dst = np.repeat(np.arange(x.shape[0]), k)
    order = np.lexsort((dst, src))
    return src[order], dst[order]


@pytest.fixture(scope="module")
def clouds():
    k = 4
    TQ, _, _ = tile(3, k)
    segs = [TQ + 5, 9, k, 40]
    x = grid_points(np.random.default_rng(9), sum(segs), 3)
    return x, segs, k, ref_edges(x, segs, k)


def test_segmented_graph(clouds):
    x, segs, k, (r_src, r_dst) = clouds
    n = x.shape[0]
    xt = th.from_numpy(x).to(DEV).requires_grad_()  # the graph is not differentiable: detached
    g = dgl.segmented_knn_graph(xt, k, segs)
    src, dst = g.edges()
    np.testing.assert_array_equal(src.numpy(), r_src)
    np.testing.assert_array_equal(dst.numpy(), r_dst)
    assert g.number_of_nodes() == n and g.number_of_edges() == n * k
    assert (g.in_degrees().numpy() == k).all()
    assert g.batch_size == len(segs)
    assert list(g.batch_num_nodes) == segs and list(g.batch_num_edges) == [k * s for s in segs]
    with pytest.raises(dgl.DGLError):
        g.add_nodes(1)
    parts = dgl.unbatch(g)
    assert [p.number_of_nodes() for p in parts] == segs
    assert [p.number_of_edges() for p in parts] == [k * s for s in segs]
    off = offsets_of(segs)
    for b, p in enumerate(parts):
        ps, pd = ref_edges(x[off[b]:off[b + 1]], [segs[b]], k)
        s, d = p.edges()
        np.testing.assert_array_equal(s.numpy(), ps)
        np.testing.assert_array_equal(d.numpy(), pd)
    # the batch info serves the readouts directly
    h = th.from_numpy(np.random.default_rng(10).standard_normal((n, 5)).astype(np.float32)).to(DEV)
    pooled = MaxPooling()(g, h)
    want = th.stack([c.max(0).values for c in th.split(h, segs, 0)])
    assert th.equal(pooled, want)
    m = SegmentedKNNGraph(k)(xt, segs)
    ms, md = m.edges()
    assert th.equal(ms, src) and th.equal(md, dst) and list(m.batch_num_nodes) == segs


def test_knn_graph_2d_and_3d():
    k, B = 3, 3
    M = tile(3, k)[0] + 5
    x = grid_points(np.random.default_rng(11), B * M, 3)
    r_src, r_dst = ref_edges(x, [M] * B, k)
    x3 = th.from_numpy(x).to(DEV).reshape(B, M, 3)
    g = dgl.knn_graph(x3, k)
    src, dst = g.edges()
    np.testing.assert_array_equal(src.numpy(), r_src)  # point j of set i is node i * M + j
    np.testing.assert_array_equal(dst.numpy(), r_dst)
    assert (src // M == dst // M).all()
    assert list(g.batch_num_nodes) == [M] * B and list(g.batch_num_edges) == [k * M] * B
    assert len(dgl.unbatch(g)) == B
    m = KNNGraph(k)(x3)
    assert th.equal(m.edges()[0], src) and th.equal(m.edges()[1], dst)
    # 2-D: one set, a batch of one
    g2 = dgl.knn_graph(x3[1], k)
    s2, d2 = g2.edges()
    p_src, p_dst = ref_edges(x[M:2 * M], [M], k)
    np.testing.assert_array_equal(s2.numpy(), p_src)
    np.testing.assert_array_equal(d2.numpy(), p_dst)
    assert g2.batch_size == 1 and g2.batch_num_nodes == [M] and g2.batch_num_edges == [k * M]
    m2 = KNNGraph(k)(x3[1])
    assert th.equal(m2.edges()[0], s2) and th.equal(m2.edges()[1], d2)


def test_number_of_nodes_when_last_point_is_no_neighbour():
    x = th.zeros(10, 3, device=DEV)  # identical points: everyone's neighbours are 0, 1, 2
    g = dgl.knn_graph(x, 3)
    assert g.number_of_nodes() == 10
    src, dst = g.edges()
    assert src.max() == 2 and (g.in_degrees().numpy() == 3).all()
    g = dgl.segmented_knn_graph(x, 3, [6, 4])
    assert g.number_of_nodes() == 10 and g.edges()[0].max() == 8


def test_edgeconv_matches_host_built_graph(clouds):
    x, segs, k, (r_src, r_dst) = clouds
    n = x.shape[0]
    g = dgl.segmented_knn_graph(th.from_numpy(x).to(DEV), k, segs)
    host = dgl.DGLGraph()
    host.add_nodes(n)
    host.add_edges(r_src, r_dst)
    th.manual_seed(0)
    conv = EdgeConv(3, 8).to(DEV)
    outs = []
    for graph in (g, host):
        h = th.from_numpy(x).to(DEV).requires_grad_()
        y = conv(graph, h)
        y.backward(th.cos(th.arange(y.numel(), device=DEV, dtype=th.float32)).view_as(y))
        outs.append((y.detach(), h.grad.clone()))
    assert th.equal(outs[0][0], outs[1][0])
    assert th.equal(outs[0][1], outs[1][1])


# ---- the example ----------------------------------------------------------------------------
def test_dgcnn_example():
    out = subprocess.check_output(
        [sys.executable, os.path.join(ROOT, "examples", "dgcnn_pointcloud.py")], timeout=300)
    r = json.loads(out.decode().strip().splitlines()[-1])
    assert r["last_loss"] < r["first_loss"], r
    assert r["train_acc"] >= 0.9, r
