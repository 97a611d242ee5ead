"""NNConv without a GPU: parameter names and shapes, the aggregator check, CPU tensors
refused, the C entries listed."""
import pytest
import torch as th

import dgl
from dgl import _ffi
from dgl.nn.pytorch import NNConv


def test_nnconv_parameters():
    conv = NNConv((5, 7), 4, th.nn.Linear(3, 20), "mean", residual=True)
    want = {"edge_nn.weight": (20, 3), "edge_nn.bias": (20,), "res_fc.weight": (4, 7), "bias": (4,)}
    assert {k: tuple(v.shape) for k, v in conv.named_parameters()} == want
    plain = NNConv(4, 4, th.nn.Linear(3, 16), "sum", residual=True, bias=False)   # identity residual
    assert set(dict(plain.named_parameters())) == {"edge_nn.weight", "edge_nn.bias"}
    assert plain.fused and bool((conv.bias == 0).all())


def test_nnconv_bad_aggregator():
    with pytest.raises(KeyError):
        NNConv(5, 4, th.nn.Linear(3, 20), "median")


def test_nnconv_refuses_cpu_tensors():
    g = dgl.DGLGraph()
    g.add_nodes(4)
    g.add_edges([0, 1, 2], [1, 2, 3])
    with pytest.raises(dgl.DGLError, match="ROCm devices only"):
        NNConv(3, 2, th.nn.Linear(2, 6), "sum")(g, th.randn(4, 3), th.randn(3, 2))


def test_nnconv_entries_exported():
    assert {"DGLMINnconvOk", "DGLMINnconvChunk", "DGLMINnconvAggregate",
            "DGLMINnconvBackward"} <= set(_ffi.EXPORTED)
