"""``RandomWalkNeighborSampler`` and ``PinSAGESampler`` (``sampling/pinsage.py``): walks with
restarts from every seed, the visit counts and the top-k selection as two HIP kernels and a
device compaction; no id visits the host."""
from .. import kernel as K
from .._ffi import DGLError
from ..graph import DGLGraph
from ..heterograph import DGLHeteroGraph
from ..transform import _built_on, _device_ids
from .randomwalks import _check_seed, _count, _draw_seed, _plan, _run


class RandomWalkNeighborSampler(object):
    """PinSAGE-like neighbour sampler for any graph, given a metapath that starts and ends at
    the same node type (``pinsage.py:13-119``).

    ``sampler(seed_nodes)`` runs ``num_random_walks`` walks from every seed, each of at most
    ``random_walk_length`` traversals of ``metapath``; after every full traversal but the
    last a walk stops with probability ``random_walk_restart_prob`` (never inside a
    traversal).  The nodes reached at the end of the traversals are counted per seed, and the
    ``num_neighbors`` most visited become the seed's neighbours.  It returns a homogeneous
    graph over ``G.number_of_nodes(ntype)`` nodes with one edge neighbour -> seed per
    selected neighbour and ``edata[weight_column]`` (device int64) holding the visit counts.
    The edges come seed by seed in the order given; a seed's edges by count descending, then
    by neighbour id ascending.

    ``metapath=None``: ``G`` has one relation over one node type (a DGLGraph, ``dgl.graph``).

    Deviation from the reference: every seed slot is counted on its own, so a seed given
    twice yields its edges twice (with the same or different counts: the two slots walk with
    different draws).  The reference pools the walks of equal seeds through ``to_simple``.

    ``seed`` (an extension): with an int, call number n of this sampler (n = 0, 1, ..) is a
    function of (graph, seed_nodes, seed, n) alone: it walks with the generator counter n *
    (walk length), see ``include/dglmi.h``.  None takes a fresh 63-bit value from torch's
    default CPU generator on every call.

    ``num_neighbors`` above ``dgl.kernel.visit_max_k()``, or ``num_random_walks *
    random_walk_length`` above ``dgl.kernel.visit_max_width()``, raise a DGLError."""

    def __init__(self, G, random_walk_length, random_walk_restart_prob, num_random_walks,
                 num_neighbors, metapath=None, weight_column="weights", seed=None):
        what = type(self).__name__
        self.G = G
        self.weight_column = weight_column
        self.random_walk_length = _count(random_walk_length, what, "random_walk_length")
        self.num_random_walks = _count(num_random_walks, what, "num_random_walks")
        self.num_neighbors = _count(num_neighbors, what, "num_neighbors")
        if min(self.random_walk_length, self.num_random_walks, self.num_neighbors) < 1:
            raise DGLError("%s: random_walk_length, num_random_walks and num_neighbors must be "
                           "at least 1" % what)
        if self.num_neighbors > K.visit_max_k():
            raise DGLError("%s: num_neighbors = %d is above the kernel's limit of %d"
                           % (what, self.num_neighbors, K.visit_max_k()))
        width = self.num_random_walks * self.random_walk_length
        if width > K.visit_max_width():
            raise DGLError("%s: num_random_walks * random_walk_length = %d is above the kernel's "
                           "limit of %d" % (what, width, K.visit_max_width()))
        _check_seed(seed, what)
        self.seed = seed
        self._calls = 0

        if isinstance(G, DGLGraph):
            if metapath is not None:
                raise DGLError("%s: a DGLGraph has no edge types; leave metapath out" % what)
            self.ntype, hops = "_N", 1
            self.metapath = None
        elif isinstance(G, DGLHeteroGraph):
            if metapath is None:
                if len(G.ntypes) > 1 or len(G.canonical_etypes) > 1:
                    raise DGLError("%s: metapath must be given for a graph with more than one "
                                   "node or edge type" % what)
                metapath = [G.canonical_etypes[0]]
            if isinstance(metapath, (str, bytes)) or not isinstance(metapath, (list, tuple)) \
                    or not metapath:
                raise DGLError("%s: metapath must be a non-empty list of edge types" % what)
            self.metapath = list(metapath)
            hops = len(self.metapath)
        else:
            raise DGLError("%s: expected a DGLGraph or a DGLHeteroGraph, got %s" % (what, type(G)))
        self.metapath_hops = hops
        L = hops * self.random_walk_length
        restart = [0.0] * L
        for t in range(hops, L, hops):
            restart[t] = float(random_walk_restart_prob)
        self.restart_prob = restart
        if self.metapath is None:
            self._plan = _plan(G, None, L, restart, what)
        else:
            self.full_metapath = self.metapath * self.random_walk_length
            _plan(G, self.metapath, None, None, what)  # the edge types exist and chain
            start = G.to_canonical_etype(self.metapath[0])[0]
            end = G.to_canonical_etype(self.metapath[-1])[2]
            if start != end:
                raise DGLError("%s: the metapath must start and end at the same node type, got "
                               "%r and %r" % (what, start, end))
            self.ntype = start
            self._plan = _plan(G, self.full_metapath, None, restart, what)

    def __call__(self, seed_nodes):
        what = type(self).__name__
        plan = self._plan
        ids, dev = _device_ids(seed_nodes, plan.n_first, _built_on(plan.rels[0]), what, "seed_nodes")
        n = int(ids.shape[0])
        if n * self.num_random_walks >= 2 ** 31:
            raise DGLError("%s: %d seeds x %d walks reach 2^31 walks" % (what, n, self.num_random_walks))
        if self.seed is None:
            seed, ctr = _draw_seed(), 0
        else:
            seed, ctr = int(self.seed), self._calls * plan.length
        self._calls += 1
        walks = ids.repeat_interleave(self.num_random_walks)
        traces = _run(plan, walks, dev, seed, ctr)
        hops = self.metapath_hops
        nbr, cnt, _ = K.visit_topk(traces, self.num_random_walks, hops, hops, self.num_neighbors)
        keep = nbr >= 0
        src = nbr[keep]  # the call's one size readback
        dst = ids.unsqueeze(1).expand_as(nbr)[keep]
        weights = cnt[keep].long()
        num = plan.n_first
        g = DGLHeteroGraph.from_device_coo((self.ntype, "_E", self.ntype), src, dst, num, num)
        g.edata[self.weight_column] = weights
        return g


class PinSAGESampler(RandomWalkNeighborSampler):
    """PinSAGE neighbour sampler on a bidirectional bipartite graph (``pinsage.py:122-216``):
    :class:`RandomWalkNeighborSampler` with the two-hop metapath ``ntype`` -> ``other_type``
    -> ``ntype``, taken from the first edge type of ``G`` in each direction."""

    def __init__(self, G, ntype, other_type, random_walk_length, random_walk_restart_prob,
                 num_random_walks, num_neighbors, weight_column="weights", seed=None):
        if not isinstance(G, DGLHeteroGraph):
            raise DGLError("PinSAGESampler: expected a DGLHeteroGraph, got %s" % type(G))

        def between(a, b):
            for c in G.canonical_etypes:
                if c[0] == a and c[2] == b:
                    return c
            raise DGLError("PinSAGESampler: no edge type from %r to %r" % (a, b))
        super().__init__(G, random_walk_length, random_walk_restart_prob, num_random_walks,
                         num_neighbors, metapath=[between(ntype, other_type),
                                                  between(other_type, ntype)],
                         weight_column=weight_column, seed=seed)
