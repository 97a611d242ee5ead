"""Message propagation along traversal frontiers (``python/dgl/propagate.py``).  The
frontiers come from ``dgl.traversal`` (device kernels); ``prop_edges_dfs`` is not provided."""
from . import traversal as trv

__all__ = ["prop_nodes", "prop_edges", "prop_nodes_bfs", "prop_nodes_topo"]


def prop_nodes(graph, nodes_generator, message_func="default", reduce_func="default",
               apply_node_func="default"):
    """Functional form of :meth:`DGLGraph.prop_nodes`."""
    graph.prop_nodes(nodes_generator, message_func, reduce_func, apply_node_func)


def prop_edges(graph, edges_generator, message_func="default", reduce_func="default",
               apply_node_func="default"):
    """Functional form of :meth:`DGLGraph.prop_edges`."""
    graph.prop_edges(edges_generator, message_func, reduce_func, apply_node_func)


def prop_nodes_bfs(graph, source, reverse=False, message_func="default", reduce_func="default",
                   apply_node_func="default"):
    """:meth:`DGLGraph.pull` on the BFS node frontiers from ``source``, in order
    (``propagate.py:57-85``)."""
    prop_nodes(graph, trv.bfs_nodes_generator(graph, source, reverse), message_func, reduce_func,
               apply_node_func)


def prop_nodes_topo(graph, reverse=False, message_func="default", reduce_func="default",
                    apply_node_func="default"):
    """:meth:`DGLGraph.pull` on the topological node frontiers, in order
    (``propagate.py:87-112``): TreeLSTM's bottom-up sweep."""
    prop_nodes(graph, trv.topological_nodes_generator(graph, reverse), message_func, reduce_func,
               apply_node_func)
