"""``RandomWalkNeighborSampler`` and ``PinSAGESampler`` on the GPU against the composed
restatement (``randomwalk_ref.pinsage``: the walks, the visit counts, the compaction): edges,
their order and their weights bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as th

import dgl

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import randomwalk_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = th.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _csr(src, dst, n):
    order = np.argsort(src, kind="stable")
    return np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))]), dst[order]


def _edges(g, column="weights"):
    src, dst = g._graph.device_uv(DEV)
    w = g.edata[column]
    assert w.dtype == th.int64 and w.device.type == "cuda"
    return src.cpu().numpy(), dst.cpu().numpy(), w.cpu().numpy()


def _same(g, want, column="weights"):
    for name, a, b in zip(("src", "dst", "weights"), _edges(g, column), want):
        assert np.array_equal(a, b), name


def _restart(hops, length, p):
    r = [0] * (hops * length)
    for t in range(hops, hops * length, hops):
        r[t] = R.threshold(p)
    return r


def _homogeneous():
    rng = np.random.default_rng(3)
    n = 60
    src, dst = rng.integers(0, n - 5, 240), rng.integers(0, n, 240)  # nodes 55 .. 59: no out-edges
    return n, src, dst


def test_homogeneous_sampler():
    n, src, dst = _homogeneous()
    host = _csr(src, dst, n)
    seeds = np.array([3, 17, 58, 3, 40, 0, 59, 21])  # a repeat and two seeds without out-edges
    for g in (dgl.graph((src, dst), num_nodes=n), None):
        if g is None:
            g = dgl.DGLGraph()
            g.add_nodes(n)
            g.add_edges(src, dst)
        sampler = dgl.sampling.RandomWalkNeighborSampler(g, 4, 0.4, 50, 6, seed=12)
        for call in range(2):  # call n walks with the counter n * length
            want = R.pinsage([host], [0] * 4, 1, seeds, 50, _restart(1, 4, 0.4), 6, 12, call * 4)
            out = sampler(th.from_numpy(seeds).to(DEV) if call else seeds)
            _same(out, want)
            assert out.number_of_nodes() == n and len(out.ntypes) == 1
            assert out.number_of_edges() == len(want[0])
        src_w, dst_w, w = want
        assert not (dst_w == 58).any() and not (dst_w == 59).any()  # no out-edges: no edges
        first, second = np.nonzero(dst_w == 3)[0][:6], np.nonzero(dst_w == 3)[0][6:]
        assert len(first) == 6 and len(second) == 6  # the repeated seed: its edges twice
    # the order inside a seed: count descending, then id ascending
    lo = 0
    for s in [3, 17, 3, 40, 0, 21]:
        hi = lo
        while hi < len(dst_w) and dst_w[hi] == s and hi - lo < 6:
            hi += 1
        keys = [(-int(w[j]), int(src_w[j])) for j in range(lo, hi)]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)
        lo = hi
    assert lo == len(dst_w)


def _bipartite():
    rng = np.random.default_rng(4)
    na, nb = 30, 45
    a, b = rng.integers(0, na - 2, 150), rng.integers(0, nb, 150)  # A nodes 28, 29: no edges
    G = dgl.heterograph({("A", "ab", "B"): (a, b), ("B", "ba", "A"): (b, a)},
                        num_nodes_dict={"A": na, "B": nb})
    return G, na, nb, _csr(a, b, na), _csr(b, a, nb)


def test_pinsage_sampler():
    G, na, nb, ab, ba = _bipartite()
    seeds = np.array([5, 0, 29, 11, 5, 27])
    sampler = dgl.sampling.PinSAGESampler(G, "A", "B", 3, 0.5, 40, 5, weight_column="visits", seed=9)
    out = sampler(seeds)
    want = R.pinsage([ab, ba], [0, 1] * 3, 2, seeds, 40, _restart(2, 3, 0.5), 5, 9)
    _same(out, want, "visits")
    assert out.number_of_nodes() == na and out.ntypes == ["A"]
    assert not (want[1] == 29).any() and (want[1] == 5).sum() == 10
    assert want[0].max() < na and want[2].max() <= 40 * 3
    # the other side: a graph over the B nodes
    other = dgl.sampling.PinSAGESampler(G, "B", "A", 2, 0.25, 30, 64, seed=10)
    seeds_b = np.arange(nb)[::-1].copy()
    want = R.pinsage([ba, ab], [0, 1] * 2, 2, seeds_b, 30, _restart(2, 2, 0.25), 64, 10)
    out = other(th.from_numpy(seeds_b).to(DEV))
    _same(out, want)
    assert out.number_of_nodes() == nb


def test_metapath_sampler_and_torch_seed():
    G, na, nb, ab, ba = _bipartite()
    S = dgl.sampling.RandomWalkNeighborSampler
    a = S(G, 2, 0.5, 20, 4, metapath=["ab", ("B", "ba", "A")], seed=3)(np.arange(10))
    want = R.pinsage([ab, ba], [0, 1] * 2, 2, np.arange(10), 20, _restart(2, 2, 0.5), 4, 3)
    _same(a, want)
    free = S(G, 2, 0.5, 20, 4, metapath=["ab", "ba"])
    th.manual_seed(21)
    x, y = free(np.arange(10)), free(np.arange(10))
    th.manual_seed(21)
    z = free(np.arange(10))
    assert all(np.array_equal(p, q) for p, q in zip(_edges(x), _edges(z)))
    assert not all(np.array_equal(p, q) for p, q in zip(_edges(x), _edges(y)))
    empty = free([])
    assert empty.number_of_edges() == 0 and empty.number_of_nodes() == na


def test_frontier_feeds_to_block():
    G, na, nb, ab, ba = _bipartite()
    seeds = th.tensor([4, 9, 1], device=DEV)
    frontier = dgl.sampling.PinSAGESampler(G, "A", "B", 2, 0.5, 30, 3, seed=1)(seeds)
    block = dgl.to_block(frontier, seeds)
    assert block.dstdata[dgl.NID].tolist() == [4, 9, 1]
    assert block.number_of_edges() == frontier.number_of_edges()
    src, dst, _ = _edges(frontier)
    got = sorted(zip(block.srcdata[dgl.NID][block._graph.device_uv(DEV)[0]].tolist(),
                     block.dstdata[dgl.NID][block._graph.device_uv(DEV)[1]].tolist()))
    assert got == sorted(zip(src.tolist(), dst.tolist()))


def test_example_runs():
    out = subprocess.check_output(
        [sys.executable, os.path.join(ROOT, "examples", "pinsage_sampling.py")], timeout=300)
    assert b"ok" in out.splitlines()[-1], out[-500:]
