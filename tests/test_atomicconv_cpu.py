"""AtomicConv and CFConv without a GPU: parameter names and shapes as the reference, the C
entries, the shapes served."""
import pytest
import torch as th

from dgl import _ffi, kernel as K
from dgl.nn.pytorch import AtomicConv, CFConv


def test_atomicconv_parameters():
    conv = AtomicConv(th.rand(5), th.rand(5), th.rand(5), th.tensor([6.0, 8.0, 1.0]))
    want = {"radial_pooling.interaction_cutoffs": (5, 1, 1), "radial_pooling.rbf_kernel_means": (5, 1, 1),
            "radial_pooling.rbf_kernel_scaling": (5, 1, 1), "features_to_use": (3,)}
    assert {k: tuple(v.shape) for k, v in conv.named_parameters()} == want
    assert conv.num_channels == 3 and conv.fused and not conv.features_to_use.requires_grad
    plain = AtomicConv(th.rand(2), th.rand(2), th.rand(2))
    assert plain.num_channels == 1 and plain.features_to_use is None


def test_cfconv_parameters():
    want = {"project_edge.0.weight": (6, 3), "project_edge.0.bias": (6,), "project_edge.2.weight": (6, 6),
            "project_edge.2.bias": (6,), "project_node.weight": (6, 4), "project_node.bias": (6,),
            "project_out.0.weight": (2, 6), "project_out.0.bias": (2,)}
    assert {k: tuple(v.shape) for k, v in CFConv(4, 3, 6, 2).named_parameters()} == want


def test_atomic_entries_exported():
    for name in ("DGLMIAtomicOk", "DGLMIAtomicChunk", "DGLMIAtomicAggregate", "DGLMIAtomicEdgeGrad"):
        assert name in _ffi.EXPORTED and hasattr(_ffi.lib(), name)
    assert _ffi.lib().DGLMIAtomicChunk() == K.ATOMIC_CHUNK


@pytest.mark.parametrize("k,t,ok", [(1, 1, True), (256, 32, True), (0, 1, False), (257, 1, False),
                                    (1, 0, False), (1, 33, False)])
def test_atomic_ok_limits(k, t, ok):
    assert K.atomic_ok(k, t) is ok
