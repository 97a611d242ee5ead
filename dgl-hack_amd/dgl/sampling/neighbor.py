"""``dgl.sampling.sample_neighbors`` and ``dgl.sampling.select_topk``: the reference's per-row
CPU picks (``sampling/neighbor.py:11-167``, ``rowwise_pick.h``, ``rowwise_sampling.cc``,
``rowwise_topk.cc``) as HIP kernels that keep every id on the device."""
import numbers

import torch as th

from .. import kernel as K
from .._ffi import DGLError
from ..transform import _built_on, _device_ids, _edge_graph, _row_owner, _single_relation


def _edge_weights(g, weight, dtypes, what, name):
    """``weight`` (an edge-feature name or a tensor) as a 1-D tensor of one value per edge of
    ``g``, unchanged in dtype and device; every error is raised here, on the host."""
    if isinstance(weight, str):
        if weight not in list(g.edata):
            raise DGLError("%s: %s names the edge feature %r, which the graph does not have%s"
                           % (what, name, weight,
                              " (weighted sampling reads its weights from it)"
                              if name == "prob" else ""))
        weight = g.edata[weight]
    if not isinstance(weight, th.Tensor):
        raise DGLError("%s: %s must be an edge feature name or a tensor, got %s"
                       % (what, name, type(weight)))
    if weight.dtype not in dtypes:
        raise DGLError("%s: %s must be of dtype %s, got %s"
                       % (what, name, " or ".join(str(d) for d in dtypes), weight.dtype))
    E = g.number_of_edges()
    if tuple(weight.shape) not in ((E,), (E, 1)):
        raise DGLError("%s: %s must have shape (%d,) or (%d, 1), one value per edge, got %s"
                       % (what, name, E, E, tuple(weight.shape)))
    return weight.detach().reshape(-1)


def _weights_on(weight, dev, what, name):
    """The weights on the graph's device ``dev``: a host tensor is copied once, a tensor on
    another device is an error."""
    if weight.device.type == "cpu":
        return weight.to(dev)
    if weight.device != dev:
        raise DGLError("%s: %s is on %s, the graph on %s" % (what, name, weight.device, dev))
    return weight


def _check_weight_device(weight, built_on, what, name):
    if weight.device.type != "cpu" and built_on is not None and weight.device != built_on:
        raise DGLError("%s: %s is on %s, the graph on %s" % (what, name, weight.device, built_on))


def _check_count(value, what, name):
    if isinstance(value, bool) or not isinstance(value, numbers.Integral):
        raise DGLError("%s: %s must be an int, got %r" % (what, name, value))
    value = int(value)
    if value < 0:
        raise DGLError("%s: %s must not be negative, got %d" % (what, name, value))
    if value > K.sample_max_fanout():
        raise DGLError("%s: %s = %d is above the kernel's limit of %d"
                       % (what, name, value, K.sample_max_fanout()))
    return value


def _frontier(g, cetype, ids, inbound, offsets, nbr, eid, n_src, n_dst):
    own = ids[_row_owner(offsets, int(nbr.shape[0])).long()]
    src, dst = (nbr, own) if inbound else (own, nbr)
    return _edge_graph(g, cetype, src, dst, n_src, n_dst, eid)


def sample_neighbors(g, nodes, fanout, edge_dir="in", prob=None, replace=False, seed=None):
    """The graph of ``g``'s nodes that keeps, for every node of ``nodes``, up to ``fanout``
    of its inbound (``edge_dir='in'``) or outbound (``'out'``) edges, drawn uniformly, or in
    proportion to ``prob``.

    ``g``: a DGLGraph, or a graph with one relation (``dgl.graph``, ``dgl.bipartite``).
    ``nodes``: an int tensor on the host or the device, or a sequence; it may repeat.
    With ``replace`` a node with any edge gets exactly ``fanout`` draws; without, a node
    with ``fanout`` edges or fewer keeps them all.  The edges come in the order of
    ``nodes``; a node's edges ascend by position in its CSR row (so by neighbour id), and
    repeats under replacement are adjacent.  ``edata[dgl.EID]`` holds the ids of the drawn
    edges in ``g`` as device int64.  ``fanout == 0`` or no nodes gives a graph without
    edges.  The result carries no CSR until a kernel asks for one.

    ``prob``: the name of an edge feature, or (an extension) a tensor: float32 or float64,
    of shape (E,) or (E, 1), on the graph's device or on the host (copied once).  Edge e is
    drawn in proportion to ``prob[e]``.  An edge whose weight is not a finite positive
    number (zero, negative, NaN, inf; float64 below 2^-900) is never drawn, and "any edge"
    and "``fanout`` edges" above count the other edges only: unlike the reference, a node
    with ``fanout`` edges or fewer does not get its zero-probability edges back.  Under
    replacement an edge below 2^-31 of the node's largest weight is never drawn.

    ``seed`` (an extension): the sample is a function of (graph, nodes, fanout, prob,
    replace, seed) alone -- ``include/dglmi.h`` states the draws.  None takes one 63-bit
    value from torch's default CPU generator, so ``torch.manual_seed`` makes a run
    reproducible and nothing synchronises with the device.

    Every error is raised on the host before anything is launched.  Ids given on the device
    are not read: one outside the graph counts as a node without edges.  One size is read
    back; no node or edge id visits the host."""
    what = "sample_neighbors"
    if edge_dir not in ("in", "out"):
        raise DGLError("sample_neighbors: edge_dir must be 'in' or 'out', got %r" % (edge_dir,))
    fanout = _check_count(fanout, what, "fanout")
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, numbers.Integral)):
        raise DGLError("sample_neighbors: seed must be an int or None, got %r" % (seed,))
    index, cetype, n_src, n_dst = _single_relation(g, what)
    built_on = _built_on(index)
    if prob is not None:
        prob = _edge_weights(g, prob, (th.float32, th.float64), what, "prob")
        _check_weight_device(prob, built_on, what, "prob")
    inbound = edge_dir == "in"
    ids, dev = _device_ids(nodes, n_dst if inbound else n_src, built_on, what, "nodes")
    if prob is not None:
        prob = _weights_on(prob, dev, what, "prob")
    if seed is None:
        seed = int(th.randint(0, 2 ** 63 - 1, (1,), dtype=th.int64).item())
    gidx = index.get_immutable_gidx(dev)
    csr = gidx.in_csr if inbound else gidx.out_csr
    if prob is None:
        offsets, nbr, eid = K.sample_neighbors(csr, ids, fanout, bool(replace), seed)
    else:
        offsets, nbr, eid = K.sample_neighbors_weighted(csr, ids, fanout, bool(replace), prob, seed)
    out = _frontier(g, cetype, ids, inbound, offsets, nbr, eid, n_src, n_dst)
    # what to_block needs to take the edge list as it stands
    out._sampled = {"seeds": ids, "offsets": offsets, "edge_dir": edge_dir}
    return out


def select_topk(g, k, weight, nodes=None, edge_dir="in", ascending=False):
    """The graph of ``g``'s nodes that keeps, for every node of ``nodes``, the ``k`` inbound
    (``edge_dir='in'``) or outbound (``'out'``) edges with the largest -- with ``ascending``
    the smallest -- ``weight`` (``sampling/neighbor.py:92-167``).

    ``weight``: the name of an edge feature, or (an extension) a tensor: float32, float64,
    int32 or int64, of shape (E,) or (E, 1), on the graph's device or on the host (copied
    once).  ``nodes``: as in :func:`sample_neighbors`; None means every node.  A node with
    ``k`` edges or fewer keeps them all.  The edges come in the order of ``nodes``, a node's
    edges in weight order -- also when it keeps them all, unlike the reference -- and edges
    of equal weight by position in the node's CSR row.  -0.0 equals 0.0, and a NaN ranks
    after every number in both directions.  ``edata[dgl.EID]`` holds the ids of the kept
    edges in ``g`` as device int64.

    The result does not carry the record that lets ``to_block`` take a sampled frontier's
    edge list as it stands: that path relies on a node's edges ascending by source, which a
    weight-ordered row does not do, so ``to_block`` takes its general path.

    Every error is raised on the host before anything is launched; no id visits the host."""
    what = "select_topk"
    if edge_dir not in ("in", "out"):
        raise DGLError("select_topk: edge_dir must be 'in' or 'out', got %r" % (edge_dir,))
    k = _check_count(k, what, "k")
    index, cetype, n_src, n_dst = _single_relation(g, what)
    built_on = _built_on(index)
    weight = _edge_weights(g, weight, (th.float32, th.float64, th.int32, th.int64), what, "weight")
    _check_weight_device(weight, built_on, what, "weight")
    inbound = edge_dir == "in"
    limit = n_dst if inbound else n_src
    if nodes is None:
        nodes = th.arange(limit, dtype=th.int32)
    ids, dev = _device_ids(nodes, limit, built_on, what, "nodes")
    weight = _weights_on(weight, dev, what, "weight")
    gidx = index.get_immutable_gidx(dev)
    offsets, nbr, eid = K.select_topk(gidx.in_csr if inbound else gidx.out_csr, ids, k, weight,
                                      bool(ascending))
    return _frontier(g, cetype, ids, inbound, offsets, nbr, eid, n_src, n_dst)
