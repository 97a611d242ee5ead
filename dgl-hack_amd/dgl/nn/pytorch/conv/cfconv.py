"""CFConv, SchNet's continuous-filter convolution, and its activation ShiftedSoftplus
(``python/dgl/nn/pytorch/conv/cfconv.py:8-97``).

Same constructor, parameters (``project_edge.{0,2}``, ``project_node``, ``project_out.0``) and
``forward(g, node_feats, edge_feats)`` as the reference.  The aggregation is u_mul_e + sum,
which the generic kernels serve forward and backward: no kernel of its own.
"""
import numpy as np
from torch import nn

from .... import function as fn


class ShiftedSoftplus(nn.Module):
    """softplus(x; beta, threshold) - log(shift)."""

    def __init__(self, beta=1, shift=2, threshold=20):
        super(ShiftedSoftplus, self).__init__()
        self.shift = shift
        self.softplus = nn.Softplus(beta=beta, threshold=threshold)

    def forward(self, inputs):
        return self.softplus(inputs) - np.log(float(self.shift))


class CFConv(nn.Module):
    def __init__(self, node_in_feats, edge_in_feats, hidden_feats, out_feats):
        super(CFConv, self).__init__()
        self.project_edge = nn.Sequential(
            nn.Linear(edge_in_feats, hidden_feats), ShiftedSoftplus(),
            nn.Linear(hidden_feats, hidden_feats), ShiftedSoftplus())
        self.project_node = nn.Linear(node_in_feats, hidden_feats)
        self.project_out = nn.Sequential(nn.Linear(hidden_feats, out_feats), ShiftedSoftplus())

    def forward(self, g, node_feats, edge_feats):
        g = g.local_var()
        g.ndata['hv'] = self.project_node(node_feats)
        g.edata['he'] = self.project_edge(edge_feats)
        g.update_all(fn.u_mul_e('hv', 'he', 'm'), fn.sum('m', 'h'))
        return self.project_out(g.ndata['h'])
