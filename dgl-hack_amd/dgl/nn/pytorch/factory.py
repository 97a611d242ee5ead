"""Modules that turn point sets into graphs (``python/dgl/nn/pytorch/factory.py``)."""
from torch import nn

from ...transform import knn_graph, segmented_knn_graph


class KNNGraph(nn.Module):
    """One point set (M, D), or B sets of M points each (B, M, D), into the k-NN graph
    (``factory.py:14-50``): the predecessors of a point are its ``k`` nearest points, and
    point j of set i is node i * M + j.  See :func:`dgl.knn_graph`."""

    def __init__(self, k):
        super(KNNGraph, self).__init__()
        self.k = k

    def forward(self, x):
        return knn_graph(x, self.k)


class SegmentedKNNGraph(nn.Module):
    """Point sets of different sizes, one after another in ``x`` (N, D), into the union of
    their k-NN graphs (``factory.py:53-92``); ``segs``: the sets' sizes, summing to N.  See
    :func:`dgl.segmented_knn_graph`."""

    def __init__(self, k):
        super(SegmentedKNNGraph, self).__init__()
        self.k = k

    def forward(self, x, segs):
        return segmented_knn_graph(x, self.k, segs)
