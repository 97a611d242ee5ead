"""Weighted neighbour sampling and select_topk on the GPU.

``offsets``, ``nbr`` and ``eid`` are compared bit for bit with ``weighted_sampling_ref.py``, a
restatement of include/dglmi.h; every call runs twice and the two results are compared
bitwise.  The graph of a fan-out (or k) F, with G the group width, has one row of every
degree in {0, 1, F - 1, F, F + 1, G - 1, G, G + 1, 2G - 1, 2G, 2G + 1}, and the rows named in
``_layout``: without an eligible weight, with fewer eligible weights than the fan-out in a
longer row, with exactly the fan-out, with NaN / inf / negative / subnormal / tiny weights,
with weights that span more than 2^31, with equal weights, of 5,000 entries, and of parallel
edges.  It is built by ``add_edges`` in shuffled order, so the CSR's ``data`` is not the
identity and the weights are gathered through edge ids.  Seed sets: none, one, one group short
of a wavefront (64 / G - 1), one seed over a workgroup (256 / G + 1), and every row shuffled
with repeats and ids outside the graph."""
import os
import sys

import numpy as np
import pytest
import torch as th

import dgl
from dgl import kernel as K

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_ref as R  # noqa: E402
import weighted_sampling_ref as W  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = th.device("cuda:0")
HUB = 5000
N = 5100
FANOUTS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64]
_GRAPHS = {}
_WEIGHTS = {}


def _group(f):
    g = 4
    while g < f:
        g *= 2
    return g


def _layout(F):
    """(kind, degree) of rows 0, 1, ..: the walked CSR's special rows."""
    G = _group(F)
    degs = sorted(d for d in {0, 1, F - 1, F, F + 1, G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1})
    return [("plain", d) for d in degs] + [
        ("dead", F + 2), ("few", F + 3), ("exact", F + 3), ("odd", 2 * G + 3), ("span", F + 5),
        ("equal", 3 * G), ("hub", HUB), ("parallel", 7)]


def _graph(F, direction="in", bits=32):
    """(DGLGraph, host CSR (indptr, indices, data), (src, dst), spans): ``spans[r]`` are the
    edge ids of special row r in the order its weights are generated in."""
    key = (F, direction, bits)
    if key not in _GRAPHS:
        rng = np.random.default_rng(200 + F)
        rows, cols = [], []
        for r, (kind, deg) in enumerate(_layout(F)):
            if kind == "parallel":
                cols.append(np.array([9, 40, 40, 40, 40, 41, 77]))
            else:
                cols.append(rng.choice(N, deg, replace=False))
            rows.append(np.full(deg, r))
        first_bg = len(rows)
        # background edges between the other nodes, so the other direction's rows are not trivial
        cols.append(rng.integers(0, N, 3000))
        rows.append(rng.integers(first_bg, N, 3000))
        sizes = [len(c) for c in cols]
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        order = rng.permutation(len(rows))
        eid_of = np.empty(len(rows), np.int64)
        eid_of[order] = np.arange(len(rows))  # generation index -> edge id
        spans = np.split(eid_of, np.cumsum(sizes)[:-1])
        rows, cols = rows[order], cols[order]
        g = dgl.DGLGraph()
        g.add_nodes(N)
        src, dst = (cols, rows) if direction == "in" else (rows, cols)
        g.add_edges(src, dst)
        if bits == 64:
            g._graph = g._graph.asbits(64)
        out_csr, in_csr = g._graph.host_csr()
        host = in_csr if direction == "in" else out_csr
        assert not np.array_equal(host[2], np.arange(len(rows)))  # data is not the identity
        _GRAPHS[key] = (g, host, (src, dst), spans)
    return _GRAPHS[key]


def _prob(F, dtype, direction="in", bits=32):
    """Sampling weights by edge id for the graph of F."""
    key = ("prob", F, dtype, direction, bits)
    if key not in _WEIGHTS:
        spans = _graph(F, direction, bits)[3]
        rng = np.random.default_rng(300 + F)
        w = np.zeros(sum(len(s) for s in spans), np.float64)
        tiny = ([2.0 ** -900, 2.0 ** -901, 5e-324, 2.0 ** -899, 1e-310] if dtype == np.float64
                else [1e-45, 3e-45, 1.1e-38, 2.0 ** -126, 2.0 ** -149])
        odd = [np.nan, np.inf, -np.inf, -2.5, 0.0, -0.0] + tiny + [1.0, 0.25, 3.0]
        for (kind, deg), s in zip(_layout(F) + [("plain", 3000)], spans):
            v = rng.uniform(0.1, 1.0, deg)
            if kind == "dead":
                v = np.resize([0.0, np.nan, -1.0, np.inf, -np.inf, -0.0], deg)
            elif kind in ("few", "exact"):
                nz = F - 1 if kind == "few" else F
                v[rng.permutation(deg)[nz:]] = 0.0
            elif kind == "odd":
                v = np.resize(odd, deg)
                v[len(odd):] = rng.uniform(0.1, 1.0, max(0, deg - len(odd)))
            elif kind == "span":
                v = 2.0 ** -40 * rng.uniform(1.0, 2.0, deg)
                v[deg // 2] = 1.0
            elif kind == "equal":
                v[:] = 0.37
            elif kind == "hub":
                v[rng.random(deg) < 0.1] = 0.0
            w[s] = v
        with np.errstate(over="ignore", under="ignore"):
            _WEIGHTS[key] = w.astype(dtype)
    return _WEIGHTS[key]


def _rank_weight(F, dtype, direction="in", bits=32):
    """Top-k weights by edge id: many ties everywhere, the special values in the 'odd' row."""
    key = ("rank", F, dtype, direction, bits)
    if key not in _WEIGHTS:
        spans = _graph(F, direction, bits)[3]
        rng = np.random.default_rng(400 + F)
        floating = np.issubdtype(dtype, np.floating)
        w = np.zeros(sum(len(s) for s in spans), dtype)
        if floating:
            odd = [0.0, -0.0, np.nan, np.inf, -np.inf, np.nan, 1.0, -1.0, 0.0, np.inf,
                   np.finfo(dtype).tiny / 4, -np.finfo(dtype).tiny / 4, np.finfo(dtype).max]
        else:
            info = np.iinfo(dtype)
            odd = [info.min, info.max, 0, -1, info.max, info.min + 1, info.max - 1, 1, info.min]
        for (kind, deg), s in zip(_layout(F) + [("plain", 3000)], spans):
            v = rng.integers(-6, 7, deg).astype(dtype)
            if floating:
                v = v / dtype(4)
            if kind == "odd":
                v[:min(deg, len(odd))] = np.asarray(odd, dtype)[:deg]
            elif kind == "equal":
                v[:] = 3
            elif kind == "hub":
                v = rng.integers(-40, 41, deg).astype(dtype)
            w[s] = v
        _WEIGHTS[key] = w
    return _WEIGHTS[key]


def _row_of(F, kind):
    return [k for k, _ in _layout(F)].index(kind)


def _seed_sets(F):
    G = _group(F)
    special = np.arange(len(_layout(F)))
    rng = np.random.default_rng(F)
    everything = np.concatenate([special, special[::3], [N + 3, -1, 2 ** 31 - 1, len(special) + 5]])
    sets = [np.empty(0, np.int64), np.array([_row_of(F, "hub")]), rng.permutation(everything)]
    for n in (64 // G - 1, 256 // G + 1):
        if n > 0:
            sets.append(np.resize(special[::-1], n))
    return sets


def _dev_csr(g, direction):
    gidx = g._graph.get_immutable_gidx(DEV)
    return gidx.in_csr if direction == "in" else gidx.out_csr


def _same(a, b):
    return all(th.equal(x, y) for x, y in zip(a, b))


def _check(got, want, what):
    assert got[0].dtype == th.int64 and got[1].dtype == th.int32 and got[2].dtype == th.int64
    for name, a, b in zip(("offsets", "nbr", "eid"), got, want):
        assert np.array_equal(a.cpu().numpy(), b), (name,) + what


def _check_sample_properties(got, seeds, edges, direction, weight, replace):
    """Independent of the restatement: parent edges with those ids, eligible, no repeats."""
    off, nbr, eid = (t.cpu().numpy() for t in got)
    src, dst = edges
    own = np.repeat(seeds, np.diff(off))
    near, far = (dst, src) if direction == "in" else (src, dst)
    assert np.array_equal(near[eid], own) and np.array_equal(far[eid], nbr)
    assert W.eligible(weight[eid]).all()
    for a, b in zip(off[:-1], off[1:]):
        if not replace:
            assert len(set(eid[a:b].tolist())) == b - a
        if direction == "in":  # an in-CSR row lists its sources ascending
            assert np.all(np.diff(nbr[a:b]) >= 0)


def _sampler_case(F, replace, dtype, direction, bits):
    g, (indptr, indices, data), edges, _ = _graph(F, direction, bits)
    csr = _dev_csr(g, direction)
    assert csr.bits == bits
    weight = _prob(F, dtype, direction, bits)
    wt = th.from_numpy(weight).to(DEV)
    for n, seeds in enumerate(_seed_sets(F)):
        rng_seed = 0x9E3779B97F4A7C15 + 1000 * F + n
        t = th.from_numpy(seeds.astype(np.int32)).to(DEV)
        got = K.sample_neighbors_weighted(csr, t, F, replace, wt, rng_seed)
        again = K.sample_neighbors_weighted(csr, t, F, replace, wt, rng_seed)
        assert _same(got, again)
        want = W.sample_weighted(indptr, indices, data, seeds.astype(np.int32), F, replace, weight,
                                 rng_seed)
        _check(got, want, (F, replace, dtype, direction, bits, len(seeds)))
        _check_sample_properties(got, seeds.astype(np.int32), edges, direction, weight, replace)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("replace", [False, True])
@pytest.mark.parametrize("F", FANOUTS)
def test_weighted_sampler_matches_the_restatement(F, replace, dtype):
    _sampler_case(F, replace, dtype, "in", 32)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("direction", ["in", "out"])
@pytest.mark.parametrize("replace", [False, True])
def test_weighted_sampler_directions_and_widths(replace, direction, bits):
    _sampler_case(9, replace, np.float32, direction, bits)


def _topk_case(F, ascending, dtype, direction, bits):
    g, (indptr, indices, data), edges, _ = _graph(F, direction, bits)
    csr = _dev_csr(g, direction)
    weight = _rank_weight(F, dtype, direction, bits)
    wt = th.from_numpy(weight).to(DEV)
    for seeds in _seed_sets(F):
        t = th.from_numpy(seeds.astype(np.int32)).to(DEV)
        got = K.select_topk(csr, t, F, wt, ascending)
        again = K.select_topk(csr, t, F, wt, ascending)
        assert _same(got, again)
        want = W.select_topk(indptr, indices, data, seeds.astype(np.int32), F, weight, ascending)
        _check(got, want, (F, ascending, dtype, direction, bits, len(seeds)))
        off, nbr, eid = (x.cpu().numpy() for x in got)
        src, dst = edges
        near, far = (dst, src) if direction == "in" else (src, dst)
        assert np.array_equal(near[eid], np.repeat(seeds, np.diff(off)))
        assert np.array_equal(far[eid], nbr)
        for a, b in zip(off[:-1], off[1:]):
            assert len(set(eid[a:b].tolist())) == b - a
    # all-equal weights: the first k positions of the row
    row = _row_of(F, "equal")
    t = th.tensor([row], dtype=th.int32, device=DEV)
    eid = K.select_topk(csr, t, F, wt, ascending)[2].cpu().numpy()
    start = int(indptr[row])
    assert np.array_equal(eid, data[start:start + F])


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32, np.int64])
@pytest.mark.parametrize("ascending", [False, True])
@pytest.mark.parametrize("F", FANOUTS)
def test_topk_matches_the_restatement(F, ascending, dtype):
    _topk_case(F, ascending, dtype, "in", 32)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("direction", ["in", "out"])
def test_topk_directions_and_widths(direction, bits):
    _topk_case(9, False, np.float32, direction, bits)
    _topk_case(9, True, np.int64, direction, bits)


def test_rows_that_decide_the_count():
    F = 5
    g, (indptr, indices, data), _, _ = _graph(F)
    csr = _dev_csr(g, "in")
    rows = [_row_of(F, k) for k in ("dead", "few", "exact", "equal")]
    t = th.tensor(rows, dtype=th.int32, device=DEV)
    for dtype in (np.float32, np.float64):
        wt = th.from_numpy(_prob(F, dtype)).to(DEV)
        off = K.sample_neighbors_weighted(csr, t, F, False, wt, 1)[0]
        assert th.diff(off).tolist() == [0, F - 1, F, F]  # nz < fanout < deg: the nz eligible
        off = K.sample_neighbors_weighted(csr, t, F, True, wt, 1)[0]
        assert th.diff(off).tolist() == [0, F, F, F]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_span_above_2_to_the_31(dtype):
    """One weight 1.0 among weights near 2^-40: with replacement only the large one is ever
    drawn; without, the small ones fill the rest of the fan-out."""
    F = 4
    g, (indptr, indices, data), _, spans = _graph(F)
    weight = _prob(F, dtype)
    wt = th.from_numpy(weight).to(DEV)
    row = _row_of(F, "span")
    t = th.full((300,), row, dtype=th.int32, device=DEV)
    eid = K.sample_neighbors_weighted(_dev_csr(g, "in"), t, F, True, wt, 5)[2].cpu().numpy()
    assert len(eid) == 300 * F and np.all(weight[eid] == 1.0)
    off, _, eid = (x.cpu().numpy() for x in
                   K.sample_neighbors_weighted(_dev_csr(g, "in"), t, F, False, wt, 5))
    assert np.all(np.diff(off) == F)
    small = (weight[eid] < 1e-9).reshape(300, F).sum(1)
    assert np.all(small >= F - 1) and np.all(small == F - 1)  # the large one: P(miss) ~ 2^-38


def test_counter_across_2_to_the_32():
    F = 5
    g, (indptr, indices, data), _, _ = _graph(F)
    csr = _dev_csr(g, "in")
    weight = _prob(F, np.float32)
    wt = th.from_numpy(weight).to(DEV)
    seeds = np.array([_row_of(F, "hub"), _row_of(F, "odd"), _row_of(F, "hub"), 3], np.int32)
    t = th.from_numpy(seeds).to(DEV)
    for ctr in (1, 2 ** 32 - 1, 2 ** 32 - 700, 2 ** 64 - 1):
        for replace in (False, True):
            got = K.sample_neighbors_weighted(csr, t, F, replace, wt, 3, rng_ctr=ctr)
            want = W.sample_weighted(indptr, indices, data, seeds, F, replace, weight, 3, rng_ctr=ctr)
            _check(got, want, (ctr, replace))
    off, nbr, eid = K.sample_neighbors_weighted(csr, t, 0, True, wt, 3)
    assert off.tolist() == [0] * 5 and nbr.numel() == 0 and eid.numel() == 0
    off, nbr, eid = K.select_topk(csr, t, 0, wt)
    assert off.tolist() == [0] * 5 and nbr.numel() == 0 and eid.numel() == 0


# ---- the public functions ------------------------------------------------------------
def _edges_of(sg):
    idx = sg._graph
    s, d = idx._device_only if hasattr(idx, "_device_only") else (idx._dev_src, idx._dev_dst)
    return s.cpu().numpy().astype(np.int64), d.cpu().numpy().astype(np.int64)


def _follow():
    """The reference's 'follow' test graph: edges, sampling probabilities, ranking weights."""
    g = dgl.DGLGraph()
    g.add_nodes(4)
    g.add_edges([1, 2, 3, 0, 2, 3, 0], [0, 0, 0, 1, 1, 1, 2])
    g.edata["prob"] = th.tensor([.5, .5, 0., .5, .5, 0., 1.])
    g.edata["weight"] = th.tensor([.5, .3, 0., -5., 22., 0., 1.])
    return g


@pytest.mark.parametrize("replace", [False, True])
def test_reference_known_answers_prob(replace):
    g = _follow()
    src = np.array([1, 2, 3, 0, 2, 3, 0])
    dst = np.array([0, 0, 0, 1, 1, 1, 2])
    for trial in range(10):
        sg = dgl.sampling.sample_neighbors(g, [0, 1], 2, prob="prob", replace=replace, seed=trial)
        assert sg.number_of_nodes() == 4 and sg.number_of_edges() == 4
        u, v = _edges_of(sg)
        eid = sg.edata[dgl.EID].cpu().numpy()
        assert set(v.tolist()) == {0, 1}
        assert np.array_equal(src[eid], u) and np.array_equal(dst[eid], v)
        edges = set(zip(u.tolist(), v.tolist()))
        if not replace:
            assert len(edges) == 4
        assert (3, 0) not in edges and (3, 1) not in edges
        # fan-out above the number of neighbours
        sg = dgl.sampling.sample_neighbors(g, [0, 2], 2, prob="prob", replace=replace, seed=trial)
        assert sg.number_of_edges() == (4 if replace else 3)
        u, v = _edges_of(sg)
        assert set(v.tolist()) == {0, 2} and (3, 0) not in set(zip(u.tolist(), v.tolist()))


def test_reference_known_answers_topk():
    g = _follow()
    src = np.array([1, 2, 3, 0, 2, 3, 0])
    dst = np.array([0, 0, 0, 1, 1, 1, 2])
    for nodes, want in (([0, 1], {(2, 0), (1, 0), (2, 1), (3, 1)}), ([0, 2], {(2, 0), (1, 0), (0, 2)})):
        sg = dgl.sampling.select_topk(g, 2, "weight", nodes)
        assert sg.number_of_nodes() == 4 and sg.number_of_edges() == len(want)
        u, v = _edges_of(sg)
        eid = sg.edata[dgl.EID].cpu().numpy()
        assert np.array_equal(src[eid], u) and np.array_equal(dst[eid], v)
        assert set(zip(u.tolist(), v.tolist())) == want
    # the reference's 'liked-by' relation: a bipartite graph
    b = dgl.bipartite(([2, 2, 2, 1, 1, 0], [0, 1, 2, 0, 3, 0]), "game", "liked-by", "user",
                      num_nodes=(3, 4))
    b.edata["weight"] = th.tensor([.3, .5, .2, .5, .1, .1])
    sg = dgl.sampling.select_topk(b, 2, "weight", [0, 1])
    u, v = _edges_of(sg)
    assert set(zip(u.tolist(), v.tolist())) == {(2, 0), (2, 1), (1, 0)}
    # every node, out-edges, ascending, an int weight given as a host tensor of shape (E, 1)
    sg = dgl.sampling.select_topk(g, 1, th.tensor([[5], [3], [0], [-5], [22], [0], [1]]),
                                  edge_dir="out", ascending=True)
    u, v = _edges_of(sg)
    assert list(zip(u.tolist(), v.tolist())) == [(0, 1), (1, 0), (2, 0), (3, 0)]
    assert sg.edata[dgl.EID].tolist() == [3, 0, 1, 2]


def test_public_prob_forms_agree():
    """A feature name, a device tensor, a host tensor and an (E, 1) tensor give the same bits,
    and they are the kernel binding's."""
    F = 5
    g, (indptr, indices, data), _, _ = _graph(F)
    weight = _prob(F, np.float64)
    seeds = th.tensor([_row_of(F, "hub"), 3, _row_of(F, "odd"), 0], device=DEV)
    g.edata["w64"] = th.from_numpy(weight)
    try:
        a = dgl.sampling.sample_neighbors(g, seeds, F, prob="w64", seed=77)
    finally:
        del g.edata["w64"]
    want = W.sample_weighted(indptr, indices, data, seeds.tolist(), F, False, weight, 77)
    assert np.array_equal(a.edata[dgl.EID].cpu().numpy(), want[2])
    for form in (th.from_numpy(weight).to(DEV), th.from_numpy(weight), th.from_numpy(weight).reshape(-1, 1)):
        b = dgl.sampling.sample_neighbors(g, seeds, F, prob=form, seed=77)
        assert th.equal(a.edata[dgl.EID], b.edata[dgl.EID])
        assert all(np.array_equal(x, y) for x, y in zip(_edges_of(a), _edges_of(b)))


def test_prob_none_keeps_its_bits():
    F = 5
    g, (indptr, indices, data), _, _ = _graph(F)
    seeds = np.array([_row_of(F, "hub"), 3, 4, 0, _row_of(F, "parallel")])
    for replace in (False, True):
        sg = dgl.sampling.sample_neighbors(g, th.from_numpy(seeds).to(DEV), F, replace=replace, seed=9)
        want = R.sample(indptr, indices, data, seeds, F, replace, 9)
        assert np.array_equal(sg.edata[dgl.EID].cpu().numpy(), want[2])
        assert np.array_equal(_edges_of(sg)[0], want[1])


def _block_arrays(b):
    s, d = _edges_of(b)
    return (s, d, b.srcdata[dgl.NID].cpu().numpy(), b.dstdata[dgl.NID].cpu().numpy(),
            b.number_of_src_nodes(), b.number_of_dst_nodes())


@pytest.mark.parametrize("replace", [False, True])
def test_to_block_on_a_weighted_frontier(replace):
    """The fast path on a weighted frontier equals the general path."""
    F = 8
    g = _graph(F)[0]
    weight = th.from_numpy(_prob(F, np.float32)).to(DEV)
    seeds = th.tensor([_row_of(F, "hub"), 900, 3, 0, _row_of(F, "parallel"), 4, _row_of(F, "few"),
                       _row_of(F, "dead")], device=DEV)
    fr = dgl.sampling.sample_neighbors(g, seeds, F, prob=weight, replace=replace, seed=8)
    assert not fr._graph._cache
    fast = dgl.to_block(fr, seeds)
    assert not fr._graph._cache  # the frontier's CSR was never built
    assert th.equal(fast.edata[dgl.EID], th.arange(fr.number_of_edges(), device=DEV))
    s, d = fr._graph._device_only
    slow = dgl.to_block(dgl.DGLGraph.from_device_coo(s, d, N), seeds)  # forgets the seeds
    for a, b in zip(_block_arrays(fast), _block_arrays(slow)):
        assert np.array_equal(a, b)
    assert th.equal(fast.edata[dgl.EID], slow.edata[dgl.EID])


def test_to_block_on_a_topk_frontier():
    """A top-k frontier's rows are in weight order, not source order, so it carries no record
    for the fast path; the block is the general path's and holds the frontier's edges."""
    F = 8
    g = _graph(F)[0]
    weight = th.from_numpy(_rank_weight(F, np.float32)).to(DEV)
    seeds = th.tensor([_row_of(F, "hub"), 900, 3, 0, _row_of(F, "parallel"), 4], device=DEV)
    fr = dgl.sampling.select_topk(g, F, weight, seeds)
    assert getattr(fr, "_sampled", None) is None
    fs, fd = _edges_of(fr)
    assert any(np.any(np.diff(fs[fd == v]) < 0) for v in seeds.tolist())  # not in source order
    block = dgl.to_block(fr, seeds)
    s, d = fr._graph._device_only
    twin = dgl.to_block(dgl.DGLGraph.from_device_coo(s, d, N), seeds)
    for a, b in zip(_block_arrays(block), _block_arrays(twin)):
        assert np.array_equal(a, b)
    bs, bd, nid_s, nid_d, n_s, n_d = _block_arrays(block)
    beid = block.edata[dgl.EID].cpu().numpy()
    assert np.array_equal(np.sort(beid), np.arange(len(fs)))
    assert np.array_equal(nid_s[bs], fs[beid]) and np.array_equal(nid_d[bd], fd[beid])
    assert nid_d.tolist() == seeds.tolist() and np.array_equal(nid_s[:n_d], nid_d)
    src_nodes, new_src, uniq = R.relabel(seeds.tolist(), fs[beid].tolist())
    assert np.array_equal(nid_s, src_nodes) and np.array_equal(bs, new_src)
