"""``dgl.sampling.random_walk`` and ``pack_traces``: the reference's OpenMP loop over seeds
(``sampling/randomwalks.py``, ``src/graph/sampling/randomwalks/``) as one HIP kernel with one
lane per walk that keeps every id on the device."""
import math
import numbers

import numpy as np
import torch as th

from .. import kernel as K
from .._ffi import DGLError
from ..graph import DGLGraph
from ..heterograph import DGLHeteroGraph
from ..transform import _built_on, _device_ids


class _Plan:
    """A validated walk: the distinct relations in order of first use, each step's index
    into them, the node type id of every trace column, the restart thresholds (or None) and
    the node count of the first source type."""

    def __init__(self, rels, path, types, thresholds, n_first):
        self.rels, self.path, self.types = rels, path, types
        self.thresholds, self.n_first = thresholds, n_first
        self.length = len(path)
        self._dev = {}

    def device_args(self, dev):
        """(csrs, metapath, restart) on ``dev``, built once per device."""
        key = str(dev)
        if key not in self._dev:
            csrs = [r.get_immutable_gidx(dev).out_csr for r in self.rels]
            path = th.tensor(self.path, dtype=th.int32).to(dev)
            thr = None if self.thresholds is None else \
                th.tensor(self.thresholds, dtype=th.int64).to(dev)
            self._dev[key] = (csrs, path, thr)
        return self._dev[key]


def _count(value, what, name):
    if isinstance(value, bool) or not isinstance(value, numbers.Integral):
        raise DGLError("%s: %s must be an int, got %r" % (what, name, value))
    if int(value) < 0:
        raise DGLError("%s: %s must not be negative, got %d" % (what, name, int(value)))
    return int(value)


def _thresholds(restart_prob, L, what):
    if restart_prob is None:
        return None
    if isinstance(restart_prob, bool):
        raise DGLError("%s: restart_prob must be a number or a tensor, got %r" % (what, restart_prob))
    if isinstance(restart_prob, numbers.Real):
        probs = [float(restart_prob)] * L
        scalar = True
    else:
        if isinstance(restart_prob, th.Tensor):
            arr = restart_prob.detach().cpu().numpy()
        else:
            try:
                arr = np.asarray(restart_prob)
            except Exception:
                raise DGLError("%s: restart_prob must be a number or a tensor" % what)
        if arr.dtype == np.bool_ or not (np.issubdtype(arr.dtype, np.floating)
                                         or np.issubdtype(arr.dtype, np.integer)):
            raise DGLError("%s: restart_prob must hold numbers, got %s" % (what, arr.dtype))
        if arr.ndim != 1 or arr.shape[0] != L:
            raise DGLError("%s: restart_prob has shape %s; one value per step of the walk (%d) "
                           "is needed" % (what, tuple(arr.shape), L))
        probs = [float(p) for p in arr.astype(np.float64)]
        scalar = False
    for t, p in enumerate(probs):
        if math.isnan(p) or p < 0:
            where = "" if scalar else " (step %d)" % t
            raise DGLError("%s: restart_prob%s must be a probability, got %r" % (what, where, p))
    return K.restart_thresholds(probs)


def _plan(g, metapath, length, restart_prob, what):
    """Validate everything that does not depend on the seeds; no launch, no device."""
    if isinstance(g, DGLGraph):
        if metapath is not None:
            raise DGLError("%s: a DGLGraph has no edge types; give length, not metapath" % what)
        if length is None:
            raise DGLError("%s: give either metapath or length" % what)
        L = _count(length, what, "length")
        n = g.number_of_nodes()
        return _Plan([g._graph], [0] * L, [0] * (L + 1), _thresholds(restart_prob, L, what), n)
    if not isinstance(g, DGLHeteroGraph):
        raise DGLError("%s: expected a DGLGraph or a DGLHeteroGraph, got %s" % (what, type(g)))
    if metapath is None:
        if length is None:
            raise DGLError("%s: give either metapath or length" % what)
        if len(g.canonical_etypes) != 1:
            raise DGLError("%s: the graph has %d edge types: give metapath, not length"
                           % (what, len(g.canonical_etypes)))
        cetypes = [g.canonical_etypes[0]] * _count(length, what, "length")
    else:
        if isinstance(metapath, (str, bytes)) or not isinstance(metapath, (list, tuple)):
            raise DGLError("%s: metapath must be a list of edge types" % what)
        cetypes = []
        for e in metapath:
            try:
                cetypes.append(g.to_canonical_etype(e))
            except (DGLError, TypeError):
                raise DGLError("%s: unknown edge type %r in metapath" % (what, e))
    for t in range(len(cetypes) - 1):
        if cetypes[t][2] != cetypes[t + 1][0]:
            raise DGLError("%s: metapath does not chain at step %d: %s ends at node type %r, %s "
                           "starts at %r" % (what, t + 1, cetypes[t], cetypes[t][2],
                                             cetypes[t + 1], cetypes[t + 1][0]))
    if cetypes:
        first = cetypes[0][0]
    elif len(g.ntypes) == 1:
        first = g.ntypes[0]
    else:
        raise DGLError("%s: an empty metapath on a graph with %d node types does not say where "
                       "the walks start" % (what, len(g.ntypes)))
    distinct = []
    for c in cetypes:
        if c not in distinct:
            distinct.append(c)
    if len(distinct) > K.walk_max_relations():
        raise DGLError("%s: the metapath uses %d distinct edge types, above the kernel's limit "
                       "of %d" % (what, len(distinct), K.walk_max_relations()))
    ntid = {t: i for i, t in enumerate(g.ntypes)}
    types = [ntid[first]] + [ntid[c[2]] for c in cetypes]
    rels = [g._rels[c] for c in distinct] or [g._rels[g.canonical_etypes[0]]]
    return _Plan(rels, [distinct.index(c) for c in cetypes], types,
                 _thresholds(restart_prob, len(cetypes), what), g.number_of_nodes(first))


def _check_seed(seed, what):
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, numbers.Integral)
                             or int(seed) < 0):
        raise DGLError("%s: seed must be a non-negative int or None, got %r" % (what, seed))


def _draw_seed():
    return int(th.randint(0, 2 ** 63 - 1, (1,), dtype=th.int64).item())


def _run(plan, ids, dev, seed, rng_ctr=0):
    csrs, path, thr = plan.device_args(dev)
    return K.random_walk(csrs, path, ids, thr, seed, rng_ctr)


def random_walk(g, nodes, *, metapath=None, length=None, prob=None, restart_prob=None, seed=None):
    """Uniform random walks from ``nodes``: ``(traces, types)``.

    ``g``: a DGLGraph or a graph with one relation, with ``length`` steps; or any
    DGLHeteroGraph with ``metapath``, a list of edge types (names or canonical triples) whose
    consecutive types chain.  ``nodes``: an int tensor on the host or the device, or a
    sequence; it may repeat.  A walk takes, at step t, a uniformly drawn out-edge of type
    ``metapath[t]`` of its current node; at a node without one it ends.  ``restart_prob``: a
    float, or one value per step (a tensor or a sequence): after step t the walk ends with
    that probability (the reference's with-restart and stepwise-restart entries); the
    probability is quantised to multiples of 2^-32.

    ``traces``: device int64 ``(len(nodes), L + 1)``, column 0 the seeds, -1 after a walk's
    end.  ``types``: device int64 ``(L + 1,)``, the node type id (``g.ntypes`` order) of every
    column; all 0 for a DGLGraph.

    ``seed`` (an extension): the traces are a function of (graph, nodes, metapath,
    restart_prob, seed) alone -- ``include/dglmi.h`` states the draws.  None takes one 63-bit
    value from torch's default CPU generator, so ``torch.manual_seed`` makes a run
    reproducible and nothing synchronises with the device.

    Every error is a DGLError raised on the host before anything is launched.  Ids given on
    the device are not read: one outside the graph starts a walk that ends at once.  No id
    visits the host.  Weighted walks (``prob``) are not built."""
    what = "random_walk"
    if prob is not None:
        raise DGLError("random_walk: weighted walks are not built (prob)")
    plan = _plan(g, metapath, length, restart_prob, what)
    _check_seed(seed, what)
    ids, dev = _device_ids(nodes, plan.n_first, _built_on(plan.rels[0]), what, "nodes")
    if seed is None:
        seed = _draw_seed()
    traces = _run(plan, ids, dev, seed)
    return traces, th.tensor(plan.types, dtype=th.int64).to(dev)


def pack_traces(traces, types):
    """``(concat_vids, concat_types, lengths, offsets)`` of padded ``traces``
    (``randomwalks.py:160-229``): the ids and node types without the -1 padding, trace after
    trace, each trace's length and its offset in the concatenation.  Torch operations on the
    tensors' device; the concatenation's size is the one value read back."""
    if not isinstance(traces, th.Tensor) or traces.dim() != 2:
        raise DGLError("pack_traces: traces must be a 2-D tensor")
    if not isinstance(types, th.Tensor) or types.dim() != 1 or types.shape[0] != traces.shape[1]:
        raise DGLError("pack_traces: types must hold one value per column of traces")
    types = types.to(traces.device)
    keep = traces >= 0
    lengths = keep.sum(1)
    offsets = th.cumsum(lengths, 0) - lengths
    return traces[keep], types.unsqueeze(0).expand_as(traces)[keep], lengths, offsets
