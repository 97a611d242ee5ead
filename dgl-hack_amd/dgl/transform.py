"""Graph transforms used by the conv modules (``python/dgl/transform.py``)."""
import numpy as np


def laplacian_lambda_max(g):
    """Largest eigenvalue of I - D^-1/2 A D^-1/2 (in-degree norm, clipped at 1) per
    graph, as a list (``transform.py:396-434``; an unbatched graph is a batch of
    one).  Host scipy ``eigs`` as the reference -- setup work, not on the
    message-passing path."""
    from scipy import sparse
    from scipy.sparse import linalg
    n = g.number_of_nodes()
    adj = g.adjacency_matrix_scipy().astype(float)
    deg = np.asarray(g.in_degrees().numpy(), dtype=float).clip(1)
    norm = sparse.diags(deg ** -0.5, dtype=float)
    lap = sparse.eye(n) - norm * adj * norm
    return [float(linalg.eigs(lap, 1, which="LM", return_eigenvectors=False)[0].real)]


def _new_graph(n, src, dst):
    from .graph import DGLGraph
    g = DGLGraph()
    g.add_nodes(n)
    if len(src):
        g.add_edges(np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64))
    return g


def _coo(g):
    src, dst, _ = g._graph.edges()
    return np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)


def add_self_loop(g):
    """Existing self-loops dropped, then one self-loop per node appended, edges kept
    in id order (``transform.py:486-519``)."""
    src, dst = _coo(g)
    keep = src != dst
    nodes = np.arange(g.number_of_nodes(), dtype=np.int64)
    return _new_graph(g.number_of_nodes(), np.concatenate([src[keep], nodes]),
                      np.concatenate([dst[keep], nodes]))


def remove_self_loop(g):
    """``transform.py:521-549``."""
    src, dst = _coo(g)
    keep = src != dst
    return _new_graph(g.number_of_nodes(), src[keep], dst[keep])


def reverse(g, share_ndata=False, share_edata=False):
    """Edges reversed, same ids (``transform.py:258-335``); ``share_*`` shares the
    feature frames with ``g``."""
    src, dst = _coo(g)
    rg = _new_graph(g.number_of_nodes(), dst, src)
    if share_ndata:
        rg._node_frame = g._node_frame
    if share_edata:
        rg._edge_frame = g._edge_frame
    return rg


def to_bidirected(g, readonly=True):
    """Both directions of every edge; a pair (u, v) gets max(#u->v, #v->u) edges
    each way (``graph_op.cc:332-401``), vectorised.  Edge order as the
    reference's general paths: readonly (``ToBidirectedImmutableGraph``) -- for
    each node u, its distinct neighbours (predecessors, then successors, in
    edge-id order), each v contributing v->u; mutable (``ToBidirectedMutableGraph``)
    -- for u <= v, the u->v copies then the v->u copies.  The reference tries a
    GKlib symmetric-CSR path first for readonly INPUT graphs
    (``graph_op.cc:651-654``); its edge order is not reproduced (parity unpinned
    for that case).  ``readonly=True`` returns a readonly graph."""
    src, dst = _coo(g)
    n = g.number_of_nodes()
    keys, counts = np.unique(src * n + dst, return_counts=True)

    def count(u, v):  # number of u -> v edges
        k = u * n + v
        pos = np.searchsorted(keys, k)
        pos_c = np.minimum(pos, max(len(keys) - 1, 0))
        hit = (pos < len(keys)) & (keys[pos_c] == k) if len(keys) else np.zeros(len(k), bool)
        return np.where(hit, counts[pos_c] if len(keys) else 0, 0)

    if readonly:
        m = len(src)
        # per node u: predecessors (phase 0) then successors (phase 1), edge-id order
        u = np.concatenate([dst, src])
        v = np.concatenate([src, dst])
        order = np.lexsort((np.arange(2 * m), np.repeat([0, 1], m), u))
        u, v = u[order], v[order]
        _, first = np.unique(u * n + v, return_index=True)
        first.sort()
        u, v = u[first], v[first]
        k = np.maximum(count(u, v), count(v, u))
        out_s, out_d = np.repeat(v, k), np.repeat(u, k)
    else:
        a, b = np.minimum(src, dst), np.maximum(src, dst)
        pairs = np.unique(a * n + b)
        u, v = pairs // n, pairs % n
        k = np.maximum(count(u, v), count(v, u))
        reps = np.where(u == v, k, 2 * k)
        pid = np.repeat(np.arange(len(u)), reps)
        j = np.arange(int(reps.sum())) - np.repeat(np.cumsum(reps) - reps, reps)
        first_half = j < k[pid]
        out_s = np.where(first_half, u[pid], v[pid])
        out_d = np.where(first_half, v[pid], u[pid])
    bg = _new_graph(n, out_s, out_d)
    bg._readonly = bool(readonly)
    return bg


def partition_graph_with_halo(g, node_part, num_hops):
    """Partition ``g`` by ``node_part`` into subgraphs that carry their halo
    (``transform.py:551-587``, ``_CAPI_DGLPartitionWithHalo`` /
    ``GraphOp::GetSubgraphWithHalo``, ``graph_op.cc:403-509``): partition p holds
    its nodes, their in-edges (only those from inner nodes when ``num_hops`` is 0)
    and, hop by hop, the in-edges of the nodes reached so far, up to ``num_hops``.
    Node ids keep the parent order (ascending); edges are listed as the reference
    collects them (in-edges of the inner nodes, then of each hop's new nodes, in
    in-CSR order).  Each subgraph is a readonly DGLGraph with ``parent_nid``,
    ``parent_eid``, ``ndata['inner_node']`` and ``edata['inner_edge']`` (int32).
    Host-side setup, as in the reference."""
    import torch as th
    from .graph import DGLGraph
    node_part = np.asarray(node_part.cpu() if hasattr(node_part, "cpu") else node_part,
                           dtype=np.int64)
    n = g.number_of_nodes()
    if node_part.shape[0] != n:
        raise ValueError("node_part needs one entry per node")
    _, in_csr = g._graph.host_csr()
    indptr, indices, eids = in_csr

    def in_edges(vs):
        beg, end = indptr[vs], indptr[vs + 1]
        lens = end - beg
        pos = np.repeat(beg - np.cumsum(lens) + lens, lens) + np.arange(int(lens.sum()))
        return indices[pos], np.repeat(vs, lens), eids[pos]

    out = {}
    for p in np.unique(node_part):
        nodes = np.nonzero(node_part == p)[0]
        seen = np.zeros(n, bool)
        seen[nodes] = True
        s, d, e = in_edges(nodes)
        inner_e = seen[s]
        if num_hops == 0:
            s, d, e, inner_e = s[inner_e], d[inner_e], e[inner_e], inner_e[inner_e]
        srcs, dsts, es, inn = [s], [d], [e], [inner_e]
        frontier = None
        if num_hops > 0:
            _, first = np.unique(s, return_index=True)
            cand = s[np.sort(first)]
            frontier = cand[~seen[cand]]
            seen[frontier] = True
        for _ in range(1, num_hops):
            s, d, e = in_edges(frontier)
            srcs.append(s)
            dsts.append(d)
            es.append(e)
            inn.append(np.zeros(len(s), bool))
            _, first = np.unique(s, return_index=True)
            cand = s[np.sort(first)]
            frontier = cand[~seen[cand]]
            seen[frontier] = True
        old_ids = np.nonzero(seen)[0]
        new_of = np.full(n, -1, np.int64)
        new_of[old_ids] = np.arange(len(old_ids))
        s, d = np.concatenate(srcs), np.concatenate(dsts)
        sub = _new_graph(len(old_ids), new_of[s], new_of[d])
        sub._readonly = True
        sub.parent_nid = th.from_numpy(old_ids)
        sub.parent_eid = th.from_numpy(np.concatenate(es))
        sub.ndata["inner_node"] = th.from_numpy((node_part[old_ids] == p).astype(np.int32))
        sub.edata["inner_edge"] = th.from_numpy(np.concatenate(inn).astype(np.int32))
        out[int(p)] = sub
    return out


def metis_partition(g, k, extra_cached_hops=0, method=None):
    """``dgl.transform.metis_partition`` (``transform.py:589-630``): a k-way node
    partition of the symmetrised graph, then :func:`partition_graph_with_halo`;
    every subgraph gets ``ndata['part_id']``.  METIS (``metis_partition.cc:19-66``)
    is absent here: the partition comes from the device label propagation
    (``dgl.distributed.partition_labelprop``, balanced by node count like METIS's
    default) when a GPU is present, else from the native LDG
    (``DGLMIPartitionLDG``).  ``method`` ("labelprop" | "ldg") forces one."""
    import torch as th
    from . import distributed as D
    src, dst = _coo(g)
    n = g.number_of_nodes()
    if method is None:
        method = "labelprop" if th.cuda.is_available() else "ldg"
    if k == 1:
        part = np.zeros(n, np.int64)
    elif method == "labelprop":
        from .graph_index import device_block_gidx
        dev = th.device("cuda", th.cuda.current_device())
        gidx = device_block_gidx(n, n, th.as_tensor(src, dtype=th.int32, device=dev),
                                 th.as_tensor(dst, dtype=th.int32, device=dev))
        a, _ = D.partition_labelprop(gidx, k, balance="nodes", slack=0.03)
        part = a.cpu().numpy().astype(np.int64)
    elif method == "ldg":
        part = D.partition_ldg(n, src, dst, k, slack=0.03)
    else:
        raise ValueError("unknown partition method %s" % method)
    parts = partition_graph_with_halo(g, part, extra_cached_hops)
    for pid, sub in parts.items():
        sub.ndata["part_id"] = th.from_numpy(part[sub.parent_nid.numpy()])
    return parts


def _knn_graph(x, k, segs, what):
    """The k-NN graph of the point sets ``segs`` (host ints) of ``x`` (N, D).  Everything
    is checked on the host before the first launch; no index visits the host after it."""
    import torch as th
    from . import kernel as K
    from ._ffi import DGLError
    from .graph import DGLGraph
    if not isinstance(x, th.Tensor) or x.dtype != th.float32:
        raise DGLError("%s: x must be a float32 tensor, got %s"
                       % (what, x.dtype if isinstance(x, th.Tensor) else type(x)))
    n = int(x.shape[0])
    k = int(k)
    if k < 1:
        raise DGLError("%s: k must be at least 1, got %d" % (what, k))
    if k > K.knn_max_k():
        raise DGLError("%s: k = %d is above the kernel's limit of %d neighbours"
                       % (what, k, K.knn_max_k()))
    if any(s < 0 for s in segs) or sum(segs) != n:
        raise DGLError("%s: the point sets hold %d points, x has %d rows" % (what, sum(segs), n))
    short = [s for s in segs if s < k]
    if short:
        raise DGLError("%s: a point set of %d points has fewer than k = %d" % (what, short[0], k))
    if n * k >= 2 ** 31:
        raise DGLError("%s: %d points times k = %d reaches 2^31 edges" % (what, n, k))
    if x.device.type != "cuda":
        raise DGLError("x is on %s: the MI355X engine runs on ROCm devices only" % x.device)
    x = x.detach().contiguous()  # the graph is not differentiable
    off = np.zeros(len(segs) + 1, np.int64)
    np.cumsum(np.asarray(segs, np.int64), out=off[1:])
    offsets = th.from_numpy(off).to(x.device)
    nbr = K.knn_select(x, offsets, k)
    # edges run neighbour -> point.  The reference's csr_matrix((1, (nbr, point))).tocoo()
    # numbers them in ascending (neighbour, point) order: the (N, k) table is point-major,
    # so one stable sort by neighbour gives exactly that.
    src, perm = th.sort(nbr.reshape(-1), stable=True)
    dst = th.div(perm, k, rounding_mode="floor").to(th.int32)
    g = DGLGraph.from_device_coo(src.contiguous(), dst.contiguous(), n)
    # extension: the result is a batch of its point sets (a set's sources are one
    # contiguous id range, so its k * s edges are contiguous in the edge order above)
    if len(segs) > 1:
        g._batch_num_nodes = [int(s) for s in segs]
        g._batch_num_edges = [k * int(s) for s in segs]
        g._segment_cache[("nodes", str(x.device))] = ((len(segs), n), offsets)
    return g


def knn_graph(x, k):
    """The graph whose nodes are the points ``x`` and in which the predecessors of a point
    are its ``k`` nearest points, itself included (``transform.py:55-98``).  ``x``: (M, D),
    or (B, M, D) for B point sets of M points each, whose graphs are unioned: point j of
    set i is node i * M + j.  Edge ids are the reference's: ascending (source, destination).

    Built on the device by one fused distance / selection kernel (``dgl.kernel.knn_select``);
    the distance is sum_f (a_f - b_f)^2, not the reference's |a|^2 + |b|^2 - 2 a.b, and ties
    go to the lower node id.  The graph is read-only, has ``x.shape[0]`` (x B) nodes whatever
    the largest neighbour id, and -- an extension -- is a batch of its B point sets
    (``batch_num_nodes`` = M each, ``batch_num_edges`` = k M each), so ``dgl.max_nodes``,
    ``MaxPooling`` and ``dgl.unbatch`` work on it directly."""
    import torch as th
    from ._ffi import DGLError
    if not isinstance(x, th.Tensor) or x.dim() not in (2, 3):
        raise DGLError("knn_graph: x must be an (M, D) or (B, M, D) tensor")
    if x.dim() == 2:
        segs = [int(x.shape[0])]
    else:
        segs = [int(x.shape[1])] * int(x.shape[0])
        x = x.reshape(-1, x.shape[2])
    return _knn_graph(x, k, segs, "knn_graph")


def segmented_knn_graph(x, k, segs):
    """:func:`knn_graph` for point sets of different sizes (``transform.py:101-141``):
    ``x`` (N, D) holds the sets one after another, ``segs`` (a host iterable of ints summing
    to N) their sizes.  The result is the batch of the sets' graphs (``batch_num_nodes`` =
    ``segs``); the per-set Python loop of the reference is one kernel launch here."""
    import torch as th
    from ._ffi import DGLError
    if not isinstance(x, th.Tensor) or x.dim() != 2:
        raise DGLError("segmented_knn_graph: x must be an (N, D) tensor")
    return _knn_graph(x, k, [int(s) for s in segs], "segmented_knn_graph")


# ---- frontiers and blocks on the device (transform.py:764-1040, one node type per side) ---
def _single_relation(g, what):
    """(index, canonical edge type or None, n_src, n_dst) of a DGLGraph or a graph with one
    relation; ``index`` has ``get_immutable_gidx``."""
    from ._ffi import DGLError
    from .graph import DGLGraph
    from .heterograph import DGLHeteroGraph
    if isinstance(g, DGLGraph):
        n = g.number_of_nodes()
        return g._graph, None, n, n
    if isinstance(g, DGLHeteroGraph):
        if len(g.canonical_etypes) != 1:
            raise DGLError("%s: the graph has %d edge types; graphs with more than one edge type "
                           "are not supported" % (what, len(g.canonical_etypes)))
        rel = g._graph
        return rel, g.canonical_etypes[0], rel.n_src, rel.n_dst
    raise DGLError("%s: expected a DGLGraph or a DGLHeteroGraph, got %s" % (what, type(g)))


def _built_on(index):
    """The device a graph was built on, or None for a host-built graph."""
    pair = getattr(index, "_device_only", None)
    if pair is not None:
        return pair[0].device
    t = getattr(index, "_dev_src", None)
    return None if t is None else t.device


def _device_ids(ids, limit, device, what, name):
    """``ids`` (tensor or sequence) as a device int32 tensor.  Host ids are range-checked
    here; device ids are not read (the kernels treat an id outside the range as a node
    without edges).  ``device``: the graph's device or None.  Returns (ids, device)."""
    import torch as th
    from ._ffi import DGLError
    if isinstance(ids, th.Tensor) and ids.device.type == "cuda":
        if ids.dtype not in (th.int32, th.int64) or ids.dim() != 1:
            raise DGLError("%s: %s must be a 1-D int32 or int64 tensor" % (what, name))
        if device is not None and ids.device != device:
            raise DGLError("%s: %s is on %s, the graph on %s" % (what, name, ids.device, device))
        return ids.to(th.int32).contiguous(), ids.device
    if isinstance(ids, th.Tensor):
        if ids.is_floating_point() or ids.dtype == th.bool:
            raise DGLError("%s: %s must hold integers, got %s" % (what, name, ids.dtype))
        host = ids.detach().numpy().astype(np.int64).reshape(-1)
    else:
        host = np.asarray(ids)
        if host.size and not np.issubdtype(host.dtype, np.integer):
            raise DGLError("%s: %s must hold integers, got %s" % (what, name, host.dtype))
        host = host.astype(np.int64).reshape(-1)
    if host.size and (host.min() < 0 or host.max() >= limit):
        bad = host[(host < 0) | (host >= limit)][0]
        raise DGLError("%s: node %d of %s is out of range [0, %d)" % (what, bad, name, limit))
    if device is None:
        if not th.cuda.is_available():
            raise DGLError("%s: no ROCm device: the MI355X engine runs on ROCm devices only" % what)
        device = th.device("cuda", th.cuda.current_device())
    return th.from_numpy(host.astype(np.int32)).to(device), device


def _edge_graph(g, cetype, src, dst, n_src, n_dst, eid):
    """A graph of ``g``'s kind and node counts with the given device edges; ``eid`` (device
    int64 ids into ``g``) goes to ``edata[EID]``.  No CSR is built."""
    from .base import EID
    from .graph import DGLGraph
    from .heterograph import DGLHeteroGraph
    if cetype is None:
        out = DGLGraph.from_device_coo(src, dst, n_src)
    else:
        out = DGLHeteroGraph.from_device_coo(cetype, src, dst, n_src, n_dst)
    out.edata[EID] = eid
    return out


def _row_owner(offsets, total):
    """The slot of every output entry of a two-phase call (device int32)."""
    from .graph_index import device_expand_rows
    return device_expand_rows(offsets, total)


def _subgraph(g, nodes, inbound, what):
    from . import kernel as K
    index, cetype, n_src, n_dst = _single_relation(g, what)
    ids, dev = _device_ids(nodes, n_dst if inbound else n_src, _built_on(index), what, "nodes")
    gidx = index.get_immutable_gidx(dev)
    offsets, nbr, eid = K.csr_gather_rows(gidx.in_csr if inbound else gidx.out_csr, ids)
    own = ids[_row_owner(offsets, int(nbr.shape[0])).long()]
    src, dst = (nbr, own) if inbound else (own, nbr)
    return _edge_graph(g, cetype, src, dst, n_src, n_dst, eid)


def in_subgraph(g, nodes):
    """The graph of ``g``'s nodes that keeps only the edges into ``nodes``
    (``transform.py:968-1005``): node by node in the order given, a node's edges in in-CSR
    order (sources ascending).  ``edata[dgl.EID]`` holds their ids in ``g`` (device int64).
    Built by one device gather balanced over the output (``dgl.kernel.csr_gather_rows``); no id
    visits the host."""
    return _subgraph(g, nodes, True, "in_subgraph")


def out_subgraph(g, nodes):
    """:func:`in_subgraph` for the edges out of ``nodes`` (``transform.py:1007-1044``)."""
    return _subgraph(g, nodes, False, "out_subgraph")


def to_block(g, dst_nodes=None, include_dst_in_src=True):
    """The bipartite block of the edges of ``g`` into ``dst_nodes`` (``transform.py:764-921``
    for one node type per side).  Edges are ordered by destination, in the order given, then
    by in-CSR position.  The destination ``dst_nodes[j]`` is node j of the DST side; with
    ``include_dst_in_src`` it is node j of the SRC side too, and the other sources follow by
    first appearance, so ``X[:block.number_of_dst_nodes()]`` are the destinations' rows of a
    SRC-side feature ``X``.  On a graph whose two sides differ in type (``dgl.bipartite``)
    the destinations are never among the sources.  ``srcdata[dgl.NID]``,
    ``dstdata[dgl.NID]`` and ``edata[dgl.EID]`` are device int64 ids into ``g``.  The node
    types of the block are ``'SRC/' + utype`` and ``'DST/' + vtype``.

    ``dst_nodes`` None: every node with an in-edge, ascending.  Repeated ``dst_nodes``
    raise.  When ``g`` is the result of ``dgl.sampling.sample_neighbors(..., edge_dir='in')``
    and ``dst_nodes`` are its seeds, the frontier's edge list already is that order and no
    CSR of the frontier is built.  One size is read back; no id visits the host."""
    import torch as th
    from . import kernel as K
    from ._ffi import DGLError
    from .base import NID, EID
    from .heterograph import DGLHeteroGraph
    what = "to_block"
    index, cetype, n_src, n_dst = _single_relation(g, what)
    utype, etype, vtype = ("_N", "_E", "_N") if cetype is None else cetype
    if isinstance(dst_nodes, dict):
        if list(dst_nodes.keys()) != [vtype]:
            raise DGLError("to_block: dst_nodes must be given for node type %s alone" % vtype)
        dst_nodes = dst_nodes[vtype]
    include = bool(include_dst_in_src) and utype == vtype
    built_on = _built_on(index)
    if dst_nodes is None:
        if built_on is None and not th.cuda.is_available():
            raise DGLError("to_block: no ROCm device: the MI355X engine runs on ROCm devices only")
        dev = built_on if built_on is not None else th.device("cuda", th.cuda.current_device())
        deg = index.get_immutable_gidx(dev).in_csr.degrees()
        ids = th.nonzero(deg > 0).reshape(-1).to(th.int32)
    else:
        ids, dev = _device_ids(dst_nodes, n_dst, built_on, what, "dst_nodes")
    S = int(ids.shape[0])

    info = getattr(g, "_sampled", None)
    fast = (info is not None and info["edge_dir"] == "in" and info["seeds"].device == dev and
            int(info["seeds"].shape[0]) == S and include)
    if fast:
        # the frontier's own edge list, if the destinations are its seeds: decided on the
        # device and read back with the relabel's sizes
        src = index._device_only[0] if cetype is None else index._dev_src
        differs = (info["seeds"] != ids).any().reshape(1).long()
        src_nodes, new_src, uniq, differs = K.block_relabel(ids, src, n_src, True, extra=differs)
        if differs:
            fast = False
        else:
            if uniq != S:
                raise DGLError("to_block: dst_nodes repeats a node (%d distinct of %d)" % (uniq, S))
            E = int(src.shape[0])
            new_dst = _row_owner(info["offsets"], E)
            eid = th.arange(E, dtype=th.int64, device=dev)
    if not fast:
        gidx = index.get_immutable_gidx(dev)
        offsets, src, eid = K.csr_gather_rows(gidx.in_csr, ids)
        if not include:
            uniq = K.block_relabel(ids, src[:0], n_dst, True)[2]
            if uniq != S:
                raise DGLError("to_block: dst_nodes repeats a node (%d distinct of %d)" % (uniq, S))
        src_nodes, new_src, uniq = K.block_relabel(ids, src, n_src, include)
        if include and uniq != S:
            raise DGLError("to_block: dst_nodes repeats a node (%d distinct of %d)" % (uniq, S))
        new_dst = _row_owner(offsets, int(src.shape[0]))
    block = DGLHeteroGraph.from_device_coo(("SRC/" + utype, etype, "DST/" + vtype), new_src, new_dst,
                                           int(src_nodes.shape[0]), S)
    block.srcdata[NID] = src_nodes
    block.dstdata[NID] = ids.long()
    block.edata[EID] = eid
    return block
