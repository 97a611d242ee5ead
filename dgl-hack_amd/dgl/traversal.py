"""Graph traversal frontiers on the device (``python/dgl/traversal.py``).

``bfs_nodes_generator``, ``bfs_edges_generator`` and ``topological_nodes_generator`` return
the reference's frontiers -- the same nodes in the same order, the order its sequential queue
discovers them -- as a tuple of device int64 tensors.  They are computed from the device CSRs
by ``dgl.kernel.traverse`` (``kernels_traverse.hip``); only the frontier sizes and the error
counts visit the host.  The DFS generators are a sequential stack per source and are not
provided.
"""
import numpy as np
import torch as th

from . import kernel as K
from ._ffi import DGLError

__all__ = ["bfs_nodes_generator", "bfs_edges_generator", "topological_nodes_generator"]


def _csrs(graph, reverse, dev):
    gidx = graph._graph.get_immutable_gidx(dev)
    return (gidx.in_csr, gidx.out_csr) if reverse else (gidx.out_csr, gidx.in_csr)


def _bfs(graph, source, reverse, kind, what, variant):
    from .transform import _built_on, _device_ids
    n = graph.number_of_nodes()
    if isinstance(source, (int, np.integer)):
        source = [int(source)]
    graph._ids_1d(source, what, "source")
    ids, dev = _device_ids(source, n, _built_on(graph._graph), what, "source")
    if isinstance(source, th.Tensor) and source.is_cuda and source.dtype == th.int64:
        # _device_ids narrows device ids to int32: keep an id outside the graph outside it
        ids = th.where((source < 0) | (source >= n), th.full_like(source, -1), source).to(th.int32)
    if dev != graph._sub_device():
        raise DGLError("%s: source is on %s, the graph on %s" % (what, dev, graph._sub_device()))
    csr, opposite = _csrs(graph, reverse, dev)
    out, sections = K.traverse(csr, opposite, kind, ids, variant)
    return th.split(out, sections) if sections else ()


def bfs_nodes_generator(graph, source, reverse=False, variant=0):
    """Node frontiers of a breadth-first search from ``source`` (a list, a numpy array or a
    host or device tensor; ``traversal.py:17-52``): frontier 0 is ``source`` itself, frontier
    k + 1 the nodes first reached from frontier k, in the order the edges of frontier k reach
    them.  ``reverse``: follow in-edges.  ``variant`` forces a kernel route (0: the shipped
    choice); the frontiers do not depend on it.

    >>> g = dgl.DGLGraph()
    >>> g.add_nodes(6)
    >>> g.add_edges([0, 1, 1, 2, 2, 3], [1, 2, 3, 3, 4, 5])
    >>> dgl.bfs_nodes_generator(g, 0)
    (tensor([0]), tensor([1]), tensor([2, 3]), tensor([4, 5]))
    """
    return _bfs(graph, source, reverse, K.TRAVERSE_BFS_NODES, "bfs_nodes_generator", variant)


def bfs_edges_generator(graph, source, reverse=False, variant=0):
    """Edge frontiers of the same search (``traversal.py:54-90``): frontier k holds the ids of
    the edges along which frontier k + 1 of :func:`bfs_nodes_generator` was first reached.

    >>> dgl.bfs_edges_generator(g, 0)      # the graph above
    (tensor([0]), tensor([1, 2]), tensor([4, 5]))
    """
    return _bfs(graph, source, reverse, K.TRAVERSE_BFS_EDGES, "bfs_edges_generator", variant)


def topological_nodes_generator(graph, reverse=False, variant=0):
    """Node frontiers in topological order (``traversal.py:92-125``): frontier 0 is the nodes
    without an in-edge, frontier k + 1 the nodes whose last in-edge comes from frontier k.
    ``reverse``: the same on the reversed graph.  A loop in the graph raises DGLError.

    >>> dgl.topological_nodes_generator(g)  # the graph above
    (tensor([0]), tensor([1]), tensor([2]), tensor([3, 4]), tensor([5]))
    """
    dev = graph._sub_device()
    csr, opposite = _csrs(graph, reverse, dev)
    out, sections = K.traverse(csr, opposite, K.TRAVERSE_TOPO, None, variant)
    return th.split(out, sections) if sections else ()
