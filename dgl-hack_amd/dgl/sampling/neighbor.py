"""``dgl.sampling.sample_neighbors``: the reference's per-row CPU pick
(``sampling/neighbor.py:11-88``, ``rowwise_pick.h``) as one HIP kernel that keeps every id
on the device."""
import numbers

import torch as th

from .. import kernel as K
from .._ffi import DGLError
from ..transform import _built_on, _device_ids, _edge_graph, _row_owner, _single_relation


def sample_neighbors(g, nodes, fanout, edge_dir="in", prob=None, replace=False, seed=None):
    """The graph of ``g``'s nodes that keeps, for every node of ``nodes``, up to ``fanout``
    of its inbound (``edge_dir='in'``) or outbound (``'out'``) edges, drawn uniformly.

    ``g``: a DGLGraph, or a graph with one relation (``dgl.graph``, ``dgl.bipartite``).
    ``nodes``: an int tensor on the host or the device, or a sequence; it may repeat.
    With ``replace`` a node with any edge gets exactly ``fanout`` draws; without, a node
    with ``fanout`` edges or fewer keeps them all.  The edges come in the order of
    ``nodes``; a node's edges ascend by position in its CSR row (so by neighbour id), and
    repeats under replacement are adjacent.  ``edata[dgl.EID]`` holds the ids of the drawn
    edges in ``g`` as device int64.  ``fanout == 0`` or no nodes gives a graph without
    edges.  The result carries no CSR until a kernel asks for one.

    ``seed`` (an extension): the sample is a function of (graph, nodes, fanout, replace,
    seed) alone -- ``include/dglmi.h`` states the draws.  None takes one 63-bit value from
    torch's default CPU generator, so ``torch.manual_seed`` makes a run reproducible and
    nothing synchronises with the device.

    Every error is raised on the host before anything is launched.  Ids given on the device
    are not read: one outside the graph counts as a node without edges.  One size is read
    back; no node or edge id visits the host."""
    what = "sample_neighbors"
    if prob is not None:
        raise DGLError("sample_neighbors: weighted sampling (prob) is not built")
    if edge_dir not in ("in", "out"):
        raise DGLError("sample_neighbors: edge_dir must be 'in' or 'out', got %r" % (edge_dir,))
    if isinstance(fanout, bool) or not isinstance(fanout, numbers.Integral):
        raise DGLError("sample_neighbors: fanout must be an int, got %r" % (fanout,))
    fanout = int(fanout)
    if fanout < 0:
        raise DGLError("sample_neighbors: fanout must not be negative, got %d" % fanout)
    if fanout > K.sample_max_fanout():
        raise DGLError("sample_neighbors: fanout = %d is above the kernel's limit of %d"
                       % (fanout, K.sample_max_fanout()))
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, numbers.Integral)):
        raise DGLError("sample_neighbors: seed must be an int or None, got %r" % (seed,))
    index, cetype, n_src, n_dst = _single_relation(g, what)
    inbound = edge_dir == "in"
    ids, dev = _device_ids(nodes, n_dst if inbound else n_src, _built_on(index), what, "nodes")
    if seed is None:
        seed = int(th.randint(0, 2 ** 63 - 1, (1,), dtype=th.int64).item())
    gidx = index.get_immutable_gidx(dev)
    offsets, nbr, eid = K.sample_neighbors(gidx.in_csr if inbound else gidx.out_csr, ids, fanout,
                                           bool(replace), seed)
    own = ids[_row_owner(offsets, int(nbr.shape[0])).long()]
    src, dst = (nbr, own) if inbound else (own, nbr)
    out = _edge_graph(g, cetype, src, dst, n_src, n_dst, eid)
    # what to_block needs to take the edge list as it stands
    out._sampled = {"seeds": ids, "offsets": offsets, "edge_dir": edge_dir}
    return out
