"""GMMConv, the Gaussian mixture model convolution of MoNet
(``python/dgl/nn/pytorch/conv/gmmconv.py:12-131``).

Same parameters (``mu``, ``inv_sigma``, ``fc``, ``res_fc``, ``bias``), initialisation,
aggregators ('sum', 'mean', 'max') and ``forward(graph, feat, pseudo)`` as the
reference, pairs ``(feat_src, feat_dst)`` on bipartite graphs and blocks included.

The reference projects every source row to K * out floats, builds an (E, K, 1) weight
tensor and gathers K * out floats per edge.  'sum' and 'mean' are linear, so the fused
form (``dgl.backend.gmm_aggregate``) aggregates first -- A[v, k] =
sum_e w_k(e) x[u], `in` floats per edge, the K weights of an edge computed in registers
-- and projects A once with ``fc.weight``.  ``fused = False`` on the module restores the
reference's step order on the builtins (u_mul_e + reducer, then the sum over K); 'max',
shapes outside ``dgl.kernel.gmm_ok`` (at the input or the output width) and 64-bit
graphs take that order too.
"""
import torch as th
from torch import nn
from torch.nn import init

from .... import backend as B
from .... import function as fn
from .gatconv import Identity, expand_as_pair


class GMMConv(nn.Module):
    def __init__(self, in_feats, out_feats, dim, n_kernels, aggregator_type='sum',
                 residual=False, bias=True):
        super(GMMConv, self).__init__()
        self._in_src_feats, self._in_dst_feats = expand_as_pair(in_feats)
        self._out_feats = out_feats
        self._dim = dim
        self._n_kernels = n_kernels
        if aggregator_type not in ('sum', 'mean', 'max'):
            raise KeyError("Aggregator type {} not recognized.".format(aggregator_type))
        self._aggre_type = aggregator_type
        self._reducer = getattr(fn, aggregator_type)
        self.fused = True
        self.mu = nn.Parameter(th.Tensor(n_kernels, dim))
        self.inv_sigma = nn.Parameter(th.Tensor(n_kernels, dim))
        self.fc = nn.Linear(self._in_src_feats, n_kernels * out_feats, bias=False)
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
        init.xavier_normal_(self.fc.weight, gain=gain)
        if isinstance(self.res_fc, nn.Linear):
            init.xavier_normal_(self.res_fc.weight, gain=gain)
        init.normal_(self.mu.data, 0, 0.1)
        init.constant_(self.inv_sigma.data, 1)
        if self.bias is not None:
            init.zeros_(self.bias.data)

    def _route(self, graph, feat_src, pseudo):
        if not self.fused or self._aggre_type == 'max':
            return None
        return B.gmm_route(graph, feat_src, pseudo, self._n_kernels, self._dim, self._out_feats)

    def forward(self, graph, feat, pseudo):
        graph = graph.local_var()
        feat_src, feat_dst = expand_as_pair(feat)
        gidx = self._route(graph, feat_src, pseudo)
        if gidx is not None:
            scale = None
            if self._aggre_type == 'mean':
                degs = graph._device_degrees(feat_src.device, "in").float()
                scale = th.where(degs > 0, 1.0 / degs.clamp(min=1), th.zeros_like(degs))
            rst = B.gmm_aggregate(gidx, feat_src, pseudo, self.mu, self.inv_sigma, self.fc.weight,
                                  row_scale=scale)
        else:
            graph.srcdata['h'] = self.fc(feat_src).view(-1, self._n_kernels, self._out_feats)
            E = graph.number_of_edges()
            gaussian = -0.5 * ((pseudo.view(E, 1, self._dim) -
                                self.mu.view(1, self._n_kernels, self._dim)) ** 2)
            gaussian = gaussian * (self.inv_sigma.view(1, self._n_kernels, self._dim) ** 2)
            graph.edata['w'] = th.exp(gaussian.sum(dim=-1, keepdim=True))  # (E, K, 1)
            graph.update_all(fn.u_mul_e('h', 'w', 'm'), self._reducer('m', 'h'))
            rst = graph.dstdata['h'].sum(1)
        if self.res_fc is not None:
            rst = rst + self.res_fc(feat_dst[:rst.shape[0]])
        if self.bias is not None:
            rst = rst + self.bias
        return rst
