"""k-NN graphs without a GPU: the names, the limits and every host-side validation error of
``dgl.knn_graph`` / ``segmented_knn_graph`` / ``dgl.kernel.knn_select`` (raised before any
device call, so CPU tensors reach them)."""
import pytest
import torch as th

import dgl
from dgl import kernel as K


def test_names_are_importable():
    from dgl import knn_graph, segmented_knn_graph
    from dgl.transform import knn_graph as t_knn, segmented_knn_graph as t_seg
    from dgl.nn.pytorch import KNNGraph, SegmentedKNNGraph
    from dgl.nn.pytorch.factory import KNNGraph as f_knn, SegmentedKNNGraph as f_seg
    assert knn_graph is t_knn and segmented_knn_graph is t_seg
    assert KNNGraph is f_knn and SegmentedKNNGraph is f_seg
    assert KNNGraph(5).k == 5 and SegmentedKNNGraph(7).k == 7
    for name in ("knn_select", "knn_tile", "knn_max_k"):
        assert callable(getattr(K, name))


def test_limits():
    assert K.knn_max_k() >= 64
    for D, k in [(1, 1), (3, 20), (64, 40), (130, K.knn_max_k())]:
        t = K.knn_tile(D, k)
        assert len(t) == 3 and all(isinstance(v, int) and v > 0 for v in t), t
    with pytest.raises(dgl.DGLError, match="between 1 and %d" % K.knn_max_k()):
        K.knn_tile(3, K.knn_max_k() + 1)
    with pytest.raises(dgl.DGLError, match="between 1 and"):
        K.knn_tile(3, 0)


X = th.zeros(12, 3)


@pytest.mark.parametrize("k", [0, -1])
def test_k_below_one(k):
    with pytest.raises(dgl.DGLError, match="at least 1"):
        dgl.knn_graph(X, k)
    with pytest.raises(dgl.DGLError, match="at least 1"):
        dgl.segmented_knn_graph(X, k, [6, 6])


def test_k_above_limit_names_the_limit():
    big = th.zeros(200, 3)
    with pytest.raises(dgl.DGLError, match="limit of %d" % K.knn_max_k()):
        dgl.knn_graph(big, K.knn_max_k() + 1)
    with pytest.raises(dgl.DGLError, match="limit of %d" % K.knn_max_k()):
        dgl.segmented_knn_graph(big, K.knn_max_k() + 1, [100, 100])


def test_short_point_set():
    with pytest.raises(dgl.DGLError, match="fewer than k = 5"):
        dgl.segmented_knn_graph(X, 5, [8, 4])
    with pytest.raises(dgl.DGLError, match="fewer than k = 5"):
        dgl.segmented_knn_graph(X, 5, [6, 0, 6])
    with pytest.raises(dgl.DGLError, match="fewer than k = 13"):
        dgl.knn_graph(X, 13)
    with pytest.raises(dgl.DGLError, match="fewer than k = 7"):
        dgl.knn_graph(X.reshape(2, 6, 3), 7)


@pytest.mark.parametrize("segs", [[6, 5], [6, 7], [], [13, -1]])
def test_segs_do_not_sum_to_rows(segs):
    with pytest.raises(dgl.DGLError, match="x has 12 rows"):
        dgl.segmented_knn_graph(X, 2, segs)


def test_dtype_and_rank():
    for bad in (X.double(), X.half(), X.long()):
        with pytest.raises(dgl.DGLError, match="float32"):
            dgl.knn_graph(bad, 2)
        with pytest.raises(dgl.DGLError, match="float32"):
            dgl.segmented_knn_graph(bad, 2, [12])
    for bad in (th.zeros(12), th.zeros(2, 2, 3, 3)):
        with pytest.raises(dgl.DGLError, match=r"\(M, D\) or \(B, M, D\)"):
            dgl.knn_graph(bad, 2)
    for bad in (th.zeros(12), th.zeros(2, 6, 3)):
        with pytest.raises(dgl.DGLError, match=r"\(N, D\)"):
            dgl.segmented_knn_graph(bad, 2, [12])
    with pytest.raises(dgl.DGLError):
        dgl.knn_graph([[0.0, 1.0]], 1)


def test_too_many_edges():
    x = th.empty(2 ** 25, 1)  # never read: the check precedes every launch
    with pytest.raises(dgl.DGLError, match="2\\^31"):
        dgl.knn_graph(x, 64)
    with pytest.raises(dgl.DGLError, match="2\\^31"):
        dgl.segmented_knn_graph(x, 64, [2 ** 24, 2 ** 24])


def test_cpu_tensor():
    with pytest.raises(dgl.DGLError, match="runs on ROCm devices only"):
        dgl.knn_graph(X, 2)
    with pytest.raises(dgl.DGLError, match="runs on ROCm devices only"):
        dgl.knn_graph(X.reshape(2, 6, 3), 2)
    with pytest.raises(dgl.DGLError, match="runs on ROCm devices only"):
        dgl.segmented_knn_graph(X, 2, [4, 8])
    with pytest.raises(dgl.DGLError, match="runs on ROCm devices only"):
        K.knn_select(X, th.tensor([0, 12]), 2)
    x = X.clone().requires_grad_()
    with pytest.raises(dgl.DGLError, match="runs on ROCm devices only"):
        dgl.nn.pytorch.KNNGraph(2)(x)
    with pytest.raises(dgl.DGLError, match="runs on ROCm devices only"):
        dgl.nn.pytorch.SegmentedKNNGraph(2)(x, [12])
