"""Sequential BFS and topological frontiers over a host copy of a CSR: a queue, a visited
list and a degree countdown, written from the contract in include/dglmi.h.  ``csr`` is
(indptr, indices, data) of the walked CSR as sequences of ints."""


def bfs(csr, source, edges=False):
    """Frontiers of node ids (of edge ids when ``edges``; then without the sources)."""
    indptr, indices, data = csr
    visited = [False] * (len(indptr) - 1)
    frontier = [int(v) for v in source]
    for v in frontier:
        visited[v] = True
    nodes, eids = [], []
    while frontier:
        nodes.append(frontier)
        nxt, via = [], []
        for u in frontier:
            for k in range(indptr[u], indptr[u + 1]):
                v = int(indices[k])
                if not visited[v]:
                    visited[v] = True
                    nxt.append(v)
                    via.append(int(data[k]))
        if via:
            eids.append(via)
        frontier = nxt
    return eids if edges else nodes


def topological(csr, opposite_indptr):
    """Frontiers of node ids; ValueError when a loop keeps nodes from being listed."""
    indptr, indices, _ = csr
    n = len(indptr) - 1
    remaining = [int(opposite_indptr[v + 1] - opposite_indptr[v]) for v in range(n)]
    frontier = [v for v in range(n) if remaining[v] == 0]
    out, listed = [], 0
    while frontier:
        out.append(frontier)
        listed += len(frontier)
        nxt = []
        for u in frontier:
            for k in range(indptr[u], indptr[u + 1]):
                v = int(indices[k])
                remaining[v] -= 1
                if remaining[v] == 0:
                    nxt.append(v)
        frontier = nxt
    if listed != n:
        raise ValueError("loop")
    return out
