"""NNConv, the edge-conditioned convolution of "Neural Message Passing for Quantum
Chemistry" (``python/dgl/nn/pytorch/conv/nnconv.py:12-121``).

Same constructor, parameters (``edge_nn.*``, ``res_fc``, ``bias``), ``reset_parameters``,
aggregators ('sum', 'mean', 'max') and ``forward(graph, feat, efeat)`` as the reference,
pairs ``(feat_src, feat_dst)`` on bipartite graphs and blocks included.

The reference multiplies (N, in, 1) by the (E, in, out) output of ``edge_nn``, reduces that
to an (N, in, out) table and sums it over `in`.  'sum' and 'mean' are linear, so the fused
form (``dgl.backend.nnconv_aggregate``) takes the sum over `in` inside the
walk: one mat-vec per edge, W streamed once, no (N, in, out) table, and backwards one walk
for both gradients.  ``fused = False`` on the module restores the reference's step order
on the builtins (u_mul_e + reducer, then the sum over `in`); 'max', widths outside
``dgl.kernel.nnconv_ok``, 64-bit graphs and edge ids that are no permutation take that
order too.
"""
import torch as th
from torch import nn
from torch.nn import init

from .... import backend as B
from .... import function as fn
from .gatconv import Identity, expand_as_pair


class NNConv(nn.Module):
    def __init__(self, in_feats, out_feats, edge_func, aggregator_type, residual=False,
                 bias=True):
        super(NNConv, self).__init__()
        self._in_src_feats, self._in_dst_feats = expand_as_pair(in_feats)
        self._out_feats = out_feats
        self.edge_nn = edge_func
        if aggregator_type not in ('sum', 'mean', 'max'):
            raise KeyError('Aggregator type {} not recognized: '.format(aggregator_type))
        self.reducer = getattr(fn, aggregator_type)
        self._aggre_type = aggregator_type
        self.fused = True
        if residual:
            if self._in_dst_feats != out_feats:
                self.res_fc = nn.Linear(self._in_dst_feats, out_feats, bias=False)
            else:
                self.res_fc = Identity()
        else:
            self.register_buffer('res_fc', None)
        if bias:
            self.bias = nn.Parameter(th.Tensor(out_feats))
        else:
            self.register_buffer('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        gain = init.calculate_gain('relu')
        if self.bias is not None:
            nn.init.zeros_(self.bias)
        if isinstance(self.res_fc, nn.Linear):
            nn.init.xavier_normal_(self.res_fc.weight, gain=gain)

    def _route(self, graph, feat_src, w):
        if not self.fused or self._aggre_type == 'max':
            return None
        return B.nnconv_route(graph, feat_src, w, self._in_src_feats, self._out_feats)

    def forward(self, graph, feat, efeat):
        graph = graph.local_var()
        feat_src, feat_dst = expand_as_pair(feat)
        w = self.edge_nn(efeat).view(-1, self._in_src_feats * self._out_feats)
        gidx = self._route(graph, feat_src, w)
        if gidx is not None:
            scale = None
            if self._aggre_type == 'mean':
                degs = graph._device_degrees(feat_src.device, "in").float()
                scale = th.where(degs > 0, 1.0 / degs.clamp(min=1), th.zeros_like(degs))
            rst = B.nnconv_aggregate(gidx, feat_src, w, row_scale=scale)
        else:
            graph.srcdata['h'] = feat_src.unsqueeze(-1)                         # (N, in, 1)
            graph.edata['w'] = w.view(-1, self._in_src_feats, self._out_feats)  # (E, in, out)
            graph.update_all(fn.u_mul_e('h', 'w', 'm'), self.reducer('m', 'neigh'))
            rst = graph.dstdata['neigh'].sum(dim=1)
        if self.res_fc is not None:
            rst = rst + self.res_fc(feat_dst[:rst.shape[0]])
        if self.bias is not None:
            rst = rst + self.bias
        return rst
