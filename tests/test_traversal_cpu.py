"""The parts of dgl.traversal that need no device: the sequential reference of the GPU tests
on the reference's docstring graph, and the host-side validation errors."""
import numpy as np
import pytest

import dgl
from dgl._ffi import DGLError

import traversal_ref as R

# the six-edge graph of the reference's traversal docstrings, as out- and in-CSR
EDGES = [(0, 1), (1, 2), (1, 3), (2, 3), (2, 4), (3, 5)]


def _csr(pairs):
    order = sorted(range(len(pairs)), key=lambda e: (pairs[e][0], pairs[e][1], e))
    indptr = np.searchsorted([pairs[e][0] for e in order], np.arange(7)).tolist()
    return indptr, [pairs[e][1] for e in order], order


OUT, IN = _csr(EDGES), _csr([(v, u) for u, v in EDGES])


def test_reference_gives_the_docstring_frontiers():
    assert R.bfs(OUT, [0]) == [[0], [1], [2, 3], [4, 5]]
    assert R.bfs(OUT, [0], edges=True) == [[0], [1, 2], [4, 5]]
    assert R.topological(OUT, IN[0]) == [[0], [1], [2], [3, 4], [5]]
    assert R.topological(IN, OUT[0]) == [[4, 5], [3], [2], [1], [0]]


def test_reference_reports_a_loop():
    with pytest.raises(ValueError):
        R.topological(_csr(EDGES + [(5, 1)]), _csr([(v, u) for u, v in EDGES + [(5, 1)]])[0])


def test_the_surface_is_exported():
    for name in ("bfs_nodes_generator", "bfs_edges_generator", "topological_nodes_generator",
                 "prop_nodes", "prop_edges", "prop_nodes_bfs", "prop_nodes_topo"):
        assert callable(getattr(dgl, name))
    assert callable(dgl.DGLGraph.prop_nodes) and callable(dgl.DGLGraph.prop_edges)
    assert dgl.traversal.bfs_nodes_generator is dgl.bfs_nodes_generator
    assert dgl.propagate.prop_nodes_topo is dgl.prop_nodes_topo


@pytest.mark.parametrize("source", [[0, 6], [-1], [0.5], np.zeros((2, 2), np.int64), [[0, 1]]])
def test_host_sources_are_validated_before_any_device_work(source):
    g = dgl.DGLGraph()
    g.add_nodes(6)
    g.add_edges(*zip(*EDGES))
    with pytest.raises(DGLError, match="bfs_nodes_generator"):
        dgl.bfs_nodes_generator(g, source)
