"""GMMConv without a GPU: parameter shapes, the aggregator check, CPU tensors refused."""
import pytest
import torch as th

import dgl
from dgl.nn.pytorch import GMMConv


def test_gmmconv_parameters():
    named = dict(GMMConv((5, 7), 4, 3, 6, "mean", residual=True).named_parameters())
    want = {"mu": (6, 3), "inv_sigma": (6, 3), "fc.weight": (24, 5), "res_fc.weight": (4, 7),
            "bias": (4,)}
    assert {k: tuple(v.shape) for k, v in named.items()} == want
    plain = GMMConv(4, 4, 2, 3, residual=True, bias=False)   # in == out: identity residual
    assert set(dict(plain.named_parameters())) == {"mu", "inv_sigma", "fc.weight"}
    assert plain.fused and bool((plain.inv_sigma == 1).all())


def test_gmmconv_bad_aggregator():
    with pytest.raises(KeyError):
        GMMConv(5, 4, 3, 6, "median")


def test_gmmconv_refuses_cpu_tensors():
    g = dgl.DGLGraph()
    g.add_nodes(4)
    g.add_edges([0, 1, 2], [1, 2, 3])
    with pytest.raises(dgl.DGLError, match="ROCm devices only"):
        GMMConv(3, 2, 2, 4)(g, th.randn(4, 3), th.randn(3, 2))
