"""AtomicConv, the atomic convolution layer of "Atomic Convolutional Networks for Predicting
Protein-Ligand Binding Affinity" (``python/dgl/nn/pytorch/conv/atomicconv.py:7-228``).

Same constructor, parameters (``radial_pooling.interaction_cutoffs``,
``radial_pooling.rbf_kernel_means``, ``radial_pooling.rbf_kernel_scaling``, each (K, 1, 1),
and the frozen ``features_to_use``), ``num_channels`` and ``forward(graph, feat, distances)``
with the t-major (V, T * K) output as the reference.

The reference builds three (K, E, 1) tensors for the radial filters, an (E, T * K) message
tensor by a message UDF and sums it by a reduce UDF on degree buckets.  The fused form
(``dgl.backend.atomic_aggregate``) reads one distance per edge and the T
values of its source and computes the K filter values where they are used.  ``fused =
False`` on the module runs the reference's own steps (``RadialPooling.forward``, the two
UDFs); more than 256 filters or 32 channels, a ``feat`` that requires grad, 64-bit graphs
and edge ids that are no permutation take those steps too.
"""
import numpy as np
import torch as th
from torch import nn

from .... import backend as B


class RadialPooling(nn.Module):
    """e_k(d) = exp(-gamma_k (d - r_k)^2) * (1/2 (cos(pi d / c_k) + 1) if d <= c_k else 0)."""

    def __init__(self, interaction_cutoffs, rbf_kernel_means, rbf_kernel_scaling):
        super(RadialPooling, self).__init__()
        self.interaction_cutoffs = nn.Parameter(
            interaction_cutoffs.reshape(-1, 1, 1), requires_grad=True)
        self.rbf_kernel_means = nn.Parameter(
            rbf_kernel_means.reshape(-1, 1, 1), requires_grad=True)
        self.rbf_kernel_scaling = nn.Parameter(
            rbf_kernel_scaling.reshape(-1, 1, 1), requires_grad=True)

    def forward(self, distances):
        """(E, 1) distances -> (K, E, 1) filter values."""
        scaled = -self.rbf_kernel_scaling * (distances - self.rbf_kernel_means) ** 2
        rbf = th.exp(scaled)
        cos_values = 0.5 * (th.cos(np.pi * distances / self.interaction_cutoffs) + 1)
        cutoff_values = th.where(distances <= self.interaction_cutoffs, cos_values,
                                 th.zeros_like(cos_values))
        return rbf * cutoff_values


def msg_func(edges):
    """'m': the (E, T * K) outer products of the source features and the filter values."""
    return {'m': th.einsum('ij,ik->ijk', edges.src['hv'], edges.data['he']).view(len(edges), -1)}


def reduce_func(nodes):
    return {'hv_new': nodes.mailbox['m'].sum(1)}


class AtomicConv(nn.Module):
    def __init__(self, interaction_cutoffs, rbf_kernel_means, rbf_kernel_scaling,
                 features_to_use=None):
        super(AtomicConv, self).__init__()
        self.radial_pooling = RadialPooling(interaction_cutoffs=interaction_cutoffs,
                                            rbf_kernel_means=rbf_kernel_means,
                                            rbf_kernel_scaling=rbf_kernel_scaling)
        self.fused = True
        if features_to_use is None:
            self.num_channels = 1
            self.features_to_use = None
        else:
            self.num_channels = len(features_to_use)
            self.features_to_use = nn.Parameter(features_to_use, requires_grad=False)

    def _route(self, graph, feat, distances):
        if not self.fused:
            return None
        return B.atomic_route(graph, feat, distances,
                              self.radial_pooling.interaction_cutoffs.numel())

    def forward(self, graph, feat, distances):
        graph = graph.local_var()
        if self.features_to_use is not None:
            feat = (feat == self.features_to_use).float()                    # (V, T)
        rp = self.radial_pooling
        gidx = self._route(graph, feat, distances)
        if gidx is not None:
            return B.atomic_aggregate(gidx, feat, distances, rp.interaction_cutoffs,
                                      rp.rbf_kernel_means, rp.rbf_kernel_scaling)
        graph.ndata['hv'] = feat
        graph.edata['he'] = rp(distances).transpose(1, 0).squeeze(-1)        # (E, K)
        graph.update_all(msg_func, reduce_func)
        return graph.ndata['hv_new'].view(graph.number_of_nodes(), -1)       # (V, K * T)
