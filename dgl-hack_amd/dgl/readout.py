"""Readout functions over batched graphs (``python/dgl/readout.py``).

A batch (``dgl.batch``) keeps graph b's nodes, and its edges, in one run of rows of the
batched frames; every function here reduces, normalises or broadcasts over those runs on
the segment kernels (``dgl.backend.segment_*`` -> ``DGLMISegment*``): one pass over the
rows in position order, no atomics, the same bits on every run.  The reference sums with
``scatter_add_`` over a host-built segment id (``backend/pytorch/tensor.py:228-239``) and
pads every graph to the largest one for max and softmax (``readout.py:396-432``).

Signatures and shapes are the reference's: a graph that is no batch is a batch of one,
results are ``(B, *)``, per-row results ``(N, *)``.
"""
from __future__ import annotations

import torch as th

from . import backend as B
from . import kernel as K
from ._ffi import DGLError

__all__ = ["sum_nodes", "sum_edges", "mean_nodes", "mean_edges", "max_nodes", "max_edges",
           "softmax_nodes", "softmax_edges", "broadcast_nodes", "broadcast_edges",
           "topk_nodes", "topk_edges"]


def _frame(graph, typestr):
    return graph.ndata if typestr == "nodes" else graph.edata


def _num_rows(graph, typestr):
    return graph.number_of_nodes() if typestr == "nodes" else graph.number_of_edges()


def segments(graph, typestr, device):
    """The ``kernel.Segments`` of ``graph``'s nodes or edges on ``device`` (offsets cached
    on the graph: no host synchronisation per call)."""
    return K.Segments(graph._segments(typestr, device), _num_rows(graph, typestr))


def _sum_on(graph, typestr, feat, weight, mean=False):
    data = _frame(graph, typestr)
    x = data[feat]
    seg = segments(graph, typestr, x.device)
    if weight is None:
        return B.segment_reduce("mean" if mean else "sum", seg, x)
    w = data[weight]
    if w.numel() != x.shape[0]:
        raise DGLError("The weight field `%s` must hold one scalar per %s, got shape %s"
                       % (weight, typestr[:-1], tuple(w.shape)))
    y = B.segment_reduce("sum", seg, x, w.reshape(-1))  # the product fused into the walk
    if not mean:
        return y
    ws = B.segment_reduce("sum", seg, w.reshape(-1, 1))
    return y / ws.reshape((-1,) + (1,) * (x.dim() - 1))  # readout.py:226-229


def sum_nodes(graph, feat, weight=None):
    """Sums the node field ``feat`` of every graph of the batch, each node's row times
    its scalar in field ``weight`` when given (``readout.py:53``).  Returns ``(B, *)``."""
    return _sum_on(graph, "nodes", feat, weight)


def sum_edges(graph, feat, weight=None):
    """``sum_nodes`` over the edge field ``feat`` (``readout.py:122``)."""
    return _sum_on(graph, "edges", feat, weight)


def mean_nodes(graph, feat, weight=None):
    """Averages the node field ``feat`` per graph; with ``weight`` the weighted sum over
    the sum of the weights (``readout.py:234``).  An empty graph's row is 0."""
    return _sum_on(graph, "nodes", feat, weight, mean=True)


def mean_edges(graph, feat, weight=None):
    """``mean_nodes`` over the edge field ``feat`` (``readout.py:303``)."""
    return _sum_on(graph, "edges", feat, weight, mean=True)


def _max_on(graph, typestr, feat):
    x = _frame(graph, typestr)[feat]
    return B.segment_reduce("max", segments(graph, typestr, x.device), x)


def max_nodes(graph, feat):
    """Elementwise maximum of the node field ``feat`` per graph (``readout.py:551``); -inf
    for a graph without nodes."""
    return _max_on(graph, "nodes", feat)


def max_edges(graph, feat):
    """Elementwise maximum of the edge field ``feat`` per graph (``readout.py:607``)."""
    return _max_on(graph, "edges", feat)


def _softmax_on(graph, typestr, feat):
    x = _frame(graph, typestr)[feat]
    return B.segment_softmax(segments(graph, typestr, x.device), x)


def softmax_nodes(graph, feat):
    """Softmax of the node field ``feat`` over the nodes of each graph, per feature
    (``readout.py:665``).  Returns ``(N, *)``."""
    return _softmax_on(graph, "nodes", feat)


def softmax_edges(graph, feat):
    """Softmax of the edge field ``feat`` over the edges of each graph (``readout.py:722``)."""
    return _softmax_on(graph, "edges", feat)


def _broadcast_on(graph, typestr, feat_data):
    return B.segment_broadcast(segments(graph, typestr, feat_data.device), feat_data)


def broadcast_nodes(graph, feat_data):
    """Row b of ``feat_data`` ``(B, *)`` for every node of graph b: ``(N, *)``
    (``readout.py:780``)."""
    return _broadcast_on(graph, "nodes", feat_data)


def broadcast_edges(graph, feat_data):
    """Row b of ``feat_data`` ``(B, *)`` for every edge of graph b: ``(E, *)``
    (``readout.py:840``)."""
    return _broadcast_on(graph, "edges", feat_data)


def _pad_index(graph, typestr, device, length):
    """For every row, its place in a (B, length) padding: b * length + position in b.
    Computed on the device from the cached offsets."""
    offsets = graph._segments(typestr, device)
    n = _num_rows(graph, typestr)
    seg = th.repeat_interleave(offsets[1:] - offsets[:-1], output_size=n)
    return seg * length + (th.arange(n, device=device) - offsets[seg])


def _topk_on(graph, typestr, feat, k, descending=True, idx=None):
    x = _frame(graph, typestr)[feat]
    if x.dim() > 2:
        raise DGLError("The {} feature `{}` should have dimension less than or"
                       " equal to 2".format(typestr, feat))
    if x.dim() == 1:
        x = x.unsqueeze(1)
    hidden = x.shape[-1]
    nums = graph.batch_num_nodes if typestr == "nodes" else graph.batch_num_edges
    bsz = len(nums)
    length = max(max(nums), k)
    place = _pad_index(graph, typestr, x.device, length)
    fill = -float("inf") if descending else float("inf")
    keys = x.new_full((bsz * length, hidden), fill).index_copy(0, place, x.detach())
    keys = keys.reshape(bsz, length, hidden)
    if idx is not None:
        order = th.argsort(keys[:, :, idx], -1, descending=descending)
    else:
        order = th.argsort(keys, 1, descending=descending)
    topk_indices = order[:, :k]
    padded = x.new_zeros((bsz * length, hidden)).index_copy(0, place, x)  # zero padding
    if idx is not None:
        shift = th.arange(bsz, device=x.device).repeat_interleave(k) * length
        rows = padded[topk_indices.reshape(-1) + shift]
    else:
        padded = padded.reshape(bsz, length, hidden)
        rows = th.gather(padded, 1, topk_indices)
    return rows.reshape(bsz, k, -1), topk_indices


def topk_nodes(graph, feat, k, descending=True, idx=None):
    """Per graph, the ``k`` largest (smallest with ``descending=False``) rows of the node
    field ``feat`` ranked by feature ``idx``, or every feature sorted on its own when
    ``idx`` is None (``readout.py:902``).  Returns ``(B, k, D)`` and the indices inside
    each graph; graphs with fewer than ``k`` nodes are padded with zero rows
    (``readout.py:502-507``)."""
    return _topk_on(graph, "nodes", feat, k, descending, idx)


def topk_edges(graph, feat, k, descending=True, idx=None):
    """``topk_nodes`` over the edge field ``feat`` (``readout.py:1016``)."""
    return _topk_on(graph, "edges", feat, k, descending, idx)
