"""Global pooling modules over batched graphs (``python/dgl/nn/pytorch/glob.py``):
one vector per graph of a batch.  Constructors and parameter names are the reference's, so
its state dicts load.  Everything per node runs on the segment kernels through
``dgl.readout``; the attention poolings take the weighted sum fused into the walk
(``sum_nodes(g, 'h', 'w')``: ``feat * gate`` is never stored) and Set2Set its scores from
``segment_rowdot`` (no ``feat * broadcast(q)`` temporary).  The Set-Transformer classes
are not provided.
"""
# pylint: disable= no-member, arguments-differ, invalid-name
import torch as th
import torch.nn as nn

from ... import backend as B
from ...readout import (sum_nodes, mean_nodes, max_nodes, softmax_nodes, topk_nodes,
                        segments)

__all__ = ["SumPooling", "AvgPooling", "MaxPooling", "SortPooling", "GlobalAttentionPooling",
           "Set2Set", "WeightAndSum"]


class SumPooling(nn.Module):
    r"""Sum pooling: :math:`r^{(i)} = \sum_{k=1}^{N_i} x^{(i)}_k` (``glob.py:SumPooling``)."""

    def forward(self, graph, feat):
        """feat (N, *) -> (B, *)."""
        with graph.local_scope():
            graph.ndata["h"] = feat
            return sum_nodes(graph, "h")


class AvgPooling(nn.Module):
    r"""Average pooling: :math:`r^{(i)} = \frac{1}{N_i}\sum_k x^{(i)}_k` (``glob.py:AvgPooling``)."""

    def forward(self, graph, feat):
        with graph.local_scope():
            graph.ndata["h"] = feat
            return mean_nodes(graph, "h")


class MaxPooling(nn.Module):
    r"""Max pooling: :math:`r^{(i)} = \max_k x^{(i)}_k` (``glob.py:MaxPooling``)."""

    def forward(self, graph, feat):
        with graph.local_scope():
            graph.ndata["h"] = feat
            return max_nodes(graph, "h")


class SortPooling(nn.Module):
    """Sort pooling (Zhang et al., "An End-to-End Deep Learning Architecture for Graph
    Classification"; ``glob.py:SortPooling``): every node's features sorted ascending, the
    ``k`` nodes with the largest last feature kept per graph, zero rows for smaller graphs.
    Returns (B, k * D)."""

    def __init__(self, k):
        super(SortPooling, self).__init__()
        self.k = k

    def forward(self, graph, feat):
        with graph.local_scope():
            feat, _ = feat.sort(dim=-1)
            graph.ndata["h"] = feat
            return topk_nodes(graph, "h", self.k, idx=-1)[0].view(-1, self.k * feat.shape[-1])


class GlobalAttentionPooling(nn.Module):
    r"""Global attention pooling (Li et al., "Gated Graph Sequence Neural Networks";
    ``glob.py:GlobalAttentionPooling``):
    :math:`r^{(i)} = \sum_k \mathrm{softmax}(f_{gate}(x_k)) f_{feat}(x_k)`."""

    def __init__(self, gate_nn, feat_nn=None):
        super(GlobalAttentionPooling, self).__init__()
        self.gate_nn = gate_nn
        self.feat_nn = feat_nn

    def forward(self, graph, feat):
        with graph.local_scope():
            gate = self.gate_nn(feat)
            assert gate.shape[-1] == 1, "The output of gate_nn should have size 1 at the last axis."
            feat = self.feat_nn(feat) if self.feat_nn else feat
            graph.ndata["gate"] = gate
            graph.ndata["a"] = softmax_nodes(graph, "gate")
            graph.ndata["h"] = feat
            return sum_nodes(graph, "h", "a")


class Set2Set(nn.Module):
    """Set2Set (Vinyals et al., "Order Matters: Sequence to sequence for sets";
    ``glob.py:Set2Set``): ``n_iters`` rounds of an LSTM query, attention over each graph's
    nodes and the attention-weighted sum.  Returns (B, 2 * input_dim)."""

    def __init__(self, input_dim, n_iters, n_layers):
        super(Set2Set, self).__init__()
        self.input_dim = input_dim
        self.output_dim = 2 * input_dim
        self.n_iters = n_iters
        self.n_layers = n_layers
        self.lstm = th.nn.LSTM(self.output_dim, self.input_dim, n_layers)
        self.reset_parameters()

    def reset_parameters(self):
        self.lstm.reset_parameters()

    def forward(self, graph, feat):
        with graph.local_scope():
            batch_size = graph.batch_size
            seg = segments(graph, "nodes", feat.device)
            h = (feat.new_zeros((self.n_layers, batch_size, self.input_dim)),
                 feat.new_zeros((self.n_layers, batch_size, self.input_dim)))
            q_star = feat.new_zeros(batch_size, self.output_dim)
            for _ in range(self.n_iters):
                q, h = self.lstm(q_star.unsqueeze(0), h)
                q = q.view(batch_size, self.input_dim)
                e = B.segment_rowdot(seg, feat, q)           # (feat * broadcast(q)).sum(-1)
                alpha = B.segment_softmax(seg, e.unsqueeze(1))
                readout = B.segment_reduce("sum", seg, feat, alpha.reshape(-1))
                q_star = th.cat([q, readout], dim=-1)
            return q_star

    def extra_repr(self):
        summary = "n_iters={n_iters}"
        return summary.format(**self.__dict__)


class WeightAndSum(nn.Module):
    """A sigmoid weight per node, then the weighted sum per graph (``glob.py:WeightAndSum``)."""

    def __init__(self, in_feats):
        super(WeightAndSum, self).__init__()
        self.in_feats = in_feats
        self.atom_weighting = nn.Sequential(nn.Linear(in_feats, 1), nn.Sigmoid())

    def forward(self, g, feats):
        with g.local_scope():
            g.ndata["h"] = feats
            g.ndata["w"] = self.atom_weighting(g.ndata["h"])
            return sum_nodes(g, "h", "w")
