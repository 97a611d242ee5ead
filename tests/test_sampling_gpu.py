"""Device neighbour sampling, row gathers and blocks on the GPU.

The sampler and the relabel are compared bit for bit with ``sampling_ref.py``, a numpy
restatement of include/dglmi.h; every call runs twice and the two results are compared
bitwise.  The graph of a fan-out F has rows of degree 0, 1, F - 1, F, F + 1 and 5,000, a
row of parallel edges, and is built by ``add_edges`` in shuffled order, so the in-CSR's
``data`` is not the identity.  Seed counts are 0, 1, one group short of a wavefront (64 / G
- 1 with G the group width) and one seed over a 256-lane workgroup (256 / G + 1); seeds
repeat and come ascending, descending and shuffled."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as th

import dgl
from dgl import kernel as K
from dgl.nn.pytorch import GATConv, SAGEConv

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = th.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dict(rtol=1e-4, atol=1e-4)  # test_conv_zoo_gpu.py's
HUB = 5000
N = 5100
FANOUTS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, "max"]
_GRAPHS = {}


def _fanout(f):
    return K.sample_max_fanout() if f == "max" else f


def _group(f):
    g = 4
    while g < f:
        g *= 2
    return g


def _graph(F, direction, bits=32):
    """Rows 0 .. 6 of the walked CSR: degree 0, 1, F - 1, F, F + 1, HUB, and 7 entries of
    which 4 are one parallel edge.  Returns (DGLGraph, host CSR (indptr, indices, data))."""
    key = (F, direction, bits)
    if key not in _GRAPHS:
        rng = np.random.default_rng(100 + F)
        rows, cols = [], []
        for row, deg in ((1, 1), (2, F - 1), (3, F), (4, F + 1), (5, HUB)):
            cols.append(rng.choice(N, deg, replace=False))
            rows.append(np.full(deg, row))
        cols.append(np.array([9, 40, 40, 40, 40, 41, 77]))
        rows.append(np.full(7, 6))
        # background edges into nodes 7 .., so the other direction's rows are not trivial
        cols.append(rng.integers(0, N, 3000))
        rows.append(rng.integers(7, N, 3000))
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        order = rng.permutation(len(rows))
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
        _GRAPHS[key] = (g, host, (src, dst))
    return _GRAPHS[key]


def _seed_sets(F):
    G = _group(F)
    special = np.arange(7)
    rng = np.random.default_rng(F)
    sets = [np.empty(0, np.int64), np.array([5]), np.array([0])]
    for n in (64 // G - 1, 256 // G + 1):
        if n > 0:
            sets.append(np.resize(special, n))                     # ascending, repeated
            sets.append(np.sort(np.resize(special, n))[::-1].copy())  # descending
            sets.append(rng.integers(0, 12, n))                    # shuffled, some background
    return sets


def _dev_csr(g, direction):
    gidx = g._graph.get_immutable_gidx(DEV)
    return gidx.in_csr if direction == "in" else gidx.out_csr


def _same(a, b):
    return all(th.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("direction", ["in", "out"])
@pytest.mark.parametrize("replace", [False, True])
@pytest.mark.parametrize("F", FANOUTS)
def test_sampler_matches_the_restatement(F, replace, direction, bits):
    F = _fanout(F)
    g, (indptr, indices, data), _ = _graph(F, direction, bits)
    csr = _dev_csr(g, direction)
    assert csr.bits == bits
    for n, seeds in enumerate(_seed_sets(F)):
        rng_seed = 0x9E3779B97F4A7C15 + 1000 * F + n
        t = th.from_numpy(seeds.astype(np.int32)).to(DEV)
        got = K.sample_neighbors(csr, t, F, replace, rng_seed)
        again = K.sample_neighbors(csr, t, F, replace, rng_seed)
        assert _same(got, again)
        assert got[0].dtype == th.int64 and got[1].dtype == th.int32 and got[2].dtype == th.int64
        want = R.sample(indptr, indices, data, seeds, F, replace, rng_seed)
        for name, a, b in zip(("offsets", "nbr", "eid"), got, want):
            assert np.array_equal(a.cpu().numpy(), b), (name, F, replace, direction, len(seeds))


def test_counter_and_zero_fanout():
    g, (indptr, indices, data), _ = _graph(5, "in")
    csr = _dev_csr(g, "in")
    seeds = np.array([5, 4, 5, 3])
    t = th.from_numpy(seeds.astype(np.int32)).to(DEV)
    for ctr in (1, 2 ** 32 - 1, 2 ** 64 - 1):
        got = K.sample_neighbors(csr, t, 5, False, 3, rng_ctr=ctr)
        want = R.sample(indptr, indices, data, seeds, 5, False, 3, rng_ctr=ctr)
        assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(got, want))
    off, nbr, eid = K.sample_neighbors(csr, t, 0, True, 3)
    assert off.tolist() == [0] * 5 and nbr.numel() == 0 and eid.numel() == 0


def test_device_seed_out_of_range_is_an_empty_row():
    g, (indptr, indices, data), _ = _graph(4, "in")
    seeds = np.array([5, N, -1, 3, 2 ** 31 - 1])
    t = th.from_numpy(seeds.astype(np.int32)).to(DEV)
    got = K.sample_neighbors(_dev_csr(g, "in"), t, 4, False, 11)
    want = R.sample(indptr, indices, data, seeds, 4, False, 11)
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(got, want))
    assert got[0].tolist() == [0, 4, 4, 4, 8, 8]


# ---- properties that do not need the restatement -------------------------------------
def _edges_of(sg):
    idx = sg._graph
    s, d = idx._device_only if hasattr(idx, "_device_only") else (idx._dev_src, idx._dev_dst)
    return s.cpu().numpy().astype(np.int64), d.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("direction", ["in", "out"])
@pytest.mark.parametrize("replace", [False, True])
@pytest.mark.parametrize("F", [3, 10, 25])
def test_sampled_edges_are_parent_edges(F, replace, direction):
    g, (indptr, _, _), (psrc, pdst) = _graph(F, direction)
    seeds = np.array([5, 0, 1, 2, 3, 4, 6, 5, 8, 9])
    sg = dgl.sampling.sample_neighbors(g, th.from_numpy(seeds).to(DEV), F, edge_dir=direction,
                                       replace=replace, seed=42)
    assert sg.number_of_nodes() == g.number_of_nodes()
    s, d = _edges_of(sg)
    eid = sg.edata[dgl.EID]
    assert eid.dtype == th.int64 and eid.device.type == "cuda"
    eid = eid.cpu().numpy()
    assert np.array_equal(psrc[eid], s) and np.array_equal(pdst[eid], d)
    own = d if direction == "in" else s
    deg = np.diff(indptr)[seeds]
    cnt = np.where(deg == 0, 0, F if replace else np.minimum(deg, F))
    assert np.array_equal(own, np.repeat(seeds, cnt))  # seed order, the count rule
    if not replace:
        for a, b in zip(np.cumsum(cnt) - cnt, np.cumsum(cnt)):
            assert len(set(eid[a:b])) == b - a
    assert not sg._graph._cache  # no CSR until someone asks for one


def test_seed_argument():
    g, _, _ = _graph(10, "in")
    seeds = th.tensor([5, 5, 5], device=DEV)
    a = dgl.sampling.sample_neighbors(g, seeds, 10, seed=1).edata[dgl.EID]
    b = dgl.sampling.sample_neighbors(g, seeds, 10, seed=1).edata[dgl.EID]
    c = dgl.sampling.sample_neighbors(g, seeds, 10, seed=2).edata[dgl.EID]
    assert th.equal(a, b) and not th.equal(a, c)
    assert not th.equal(a[:10], a[10:20])  # the slot, not the node, indexes the draws
    th.manual_seed(77)
    d = dgl.sampling.sample_neighbors(g, seeds, 10).edata[dgl.EID]
    e = dgl.sampling.sample_neighbors(g, seeds, 10).edata[dgl.EID]
    th.manual_seed(77)
    f = dgl.sampling.sample_neighbors(g, seeds, 10).edata[dgl.EID]
    assert th.equal(d, f) and not th.equal(d, e)


def test_host_seeds_sequences_and_empty_results():
    g, _, _ = _graph(4, "in")
    a = dgl.sampling.sample_neighbors(g, [5, 3], 4, seed=5)
    b = dgl.sampling.sample_neighbors(g, th.tensor([5, 3]), 4, seed=5)
    c = dgl.sampling.sample_neighbors(g, th.tensor([5, 3], dtype=th.int32, device=DEV), 4, seed=5)
    assert th.equal(a.edata[dgl.EID], b.edata[dgl.EID]) and th.equal(a.edata[dgl.EID], c.edata[dgl.EID])
    assert a.number_of_edges() == 8
    for sg in (dgl.sampling.sample_neighbors(g, [5, 3], 0), dgl.sampling.sample_neighbors(g, [], 4),
               dgl.sampling.sample_neighbors(g, [0], 4)):
        assert sg.number_of_edges() == 0 and sg.number_of_nodes() == N
        assert sg.edata[dgl.EID].numel() == 0


def test_hetero_inputs():
    rng = np.random.default_rng(3)
    u, v = rng.integers(0, 50, 400), rng.integers(0, 20, 400)
    bg = dgl.bipartite((u, v), num_nodes=(50, 20))
    sg = dgl.sampling.sample_neighbors(bg, [0, 7, 19], 5, seed=9)
    assert isinstance(sg, dgl.DGLHeteroGraph) and sg.canonical_etypes == bg.canonical_etypes
    assert sg.number_of_src_nodes() == 50 and sg.number_of_dst_nodes() == 20
    s, d = _edges_of(sg)
    e = sg.edata[dgl.EID].cpu().numpy()
    assert np.array_equal(u[e], s) and np.array_equal(v[e], d) and set(d) <= {0, 7, 19}
    so = dgl.sampling.sample_neighbors(bg, [49, 3], 2, edge_dir="out", seed=9)
    s, d = _edges_of(so)
    e = so.edata[dgl.EID].cpu().numpy()
    assert np.array_equal(u[e], s) and np.array_equal(v[e], d) and set(s) <= {49, 3}
    hg = dgl.graph((u % 20, v), num_nodes=20)
    sh = dgl.sampling.sample_neighbors(hg, [1, 2], 3, seed=1)
    assert isinstance(sh, dgl.DGLHeteroGraph) and sh.number_of_nodes() == 20


# ---- gather_rows, in_subgraph, out_subgraph ---------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("direction", ["in", "out"])
def test_gather_rows(direction, bits):
    g, (indptr, indices, data), _ = _graph(9, direction, bits)
    for rows in ([], [0], [5], [5, 0, 0, 5, 1, 6, 4000, 0], list(range(300, 0, -1))):
        rows = np.asarray(rows, np.int64)
        t = th.from_numpy(rows.astype(np.int32)).to(DEV)
        got = K.csr_gather_rows(_dev_csr(g, direction), t)
        assert _same(got, K.csr_gather_rows(_dev_csr(g, direction), t))
        want = R.gather_rows(indptr, indices, data, rows)
        for a, b in zip(got, want):
            assert np.array_equal(a.cpu().numpy(), b)


@pytest.mark.parametrize("direction", ["in", "out"])
def test_subgraphs(direction):
    g, (indptr, indices, data), (psrc, pdst) = _graph(9, direction)
    nodes = np.array([5, 0, 6, 2, 0, 1000])
    fn = dgl.in_subgraph if direction == "in" else dgl.out_subgraph
    sg = fn(g, th.from_numpy(nodes).to(DEV))
    _, nbr, eid = R.gather_rows(indptr, indices, data, nodes)
    s, d = _edges_of(sg)
    own = np.repeat(nodes, np.diff(indptr)[nodes])
    assert np.array_equal(sg.edata[dgl.EID].cpu().numpy(), eid)
    assert np.array_equal(s, nbr if direction == "in" else own)
    assert np.array_equal(d, own if direction == "in" else nbr)
    assert np.array_equal(psrc[eid], s) and np.array_equal(pdst[eid], d)
    assert sg.number_of_nodes() == N
    assert fn(g, [0]).number_of_edges() == 0


# ---- to_block -----------------------------------------------------------------------------
def _table_is_free():
    t = K.relabel_table(DEV, 1)
    return bool((t == 2 ** 31 - 1).all())


def test_to_block_reference_example_homogeneous():
    g = dgl.graph([(0, 1), (1, 2), (2, 3)])
    block = dgl.to_block(g, th.LongTensor([3, 2]))
    assert block.dstdata[dgl.NID].tolist() == [3, 2]
    assert block.srcdata[dgl.NID].tolist() == [3, 2, 1]
    assert block.edata[dgl.EID].tolist() == [2, 1]
    for t in (block.dstdata[dgl.NID], block.srcdata[dgl.NID], block.edata[dgl.EID]):
        assert t.dtype == th.int64 and t.device.type == "cuda"
    src, dst = block.edges()
    assert block.srcdata[dgl.NID][src.to(DEV)].tolist() == [2, 1]
    assert block.dstdata[dgl.NID][dst.to(DEV)].tolist() == [3, 2]
    assert block.number_of_src_nodes() == 3 and block.number_of_dst_nodes() == 2
    assert _table_is_free()


def test_to_block_reference_example_bipartite():
    g = dgl.bipartite([(0, 1), (1, 2), (2, 3)], utype="A", vtype="B")
    for dst in ({"B": th.LongTensor([3, 2])}, th.LongTensor([3, 2]).to(DEV)):
        block = dgl.to_block(g, dst)
        assert block.dstdata[dgl.NID].tolist() == [3, 2]
        assert block.srcdata[dgl.NID].tolist() == [2, 1]
        assert block.edata[dgl.EID].tolist() == [2, 1]
    assert _table_is_free()


def test_to_block_without_dst_in_src_and_default_dst():
    g = dgl.DGLGraph()
    g.add_nodes(6)
    g.add_edges([0, 1, 2, 2, 5], [1, 2, 3, 3, 3])
    block = dgl.to_block(g, [3, 2], include_dst_in_src=False)
    assert block.srcdata[dgl.NID].tolist() == [2, 5, 1]
    assert block.edata[dgl.EID].tolist() == [2, 3, 4, 1]
    assert block.edges()[0].tolist() == [0, 0, 1, 2] and block.edges()[1].tolist() == [0, 0, 0, 1]
    block = dgl.to_block(g)  # every node with an in-edge, ascending
    assert block.dstdata[dgl.NID].tolist() == [1, 2, 3]
    assert block.srcdata[dgl.NID].tolist() == [1, 2, 3, 0, 5]
    assert block.edata[dgl.EID].tolist() == [0, 1, 2, 3, 4]
    assert _table_is_free()


@pytest.mark.parametrize("include", [True, False])
def test_to_block_repeated_dst_raises(include):
    g, _, _ = _graph(4, "in")
    with pytest.raises(dgl.DGLError, match="repeats a node"):
        dgl.to_block(g, [3, 5, 3], include_dst_in_src=include)
    assert _table_is_free()
    fr = dgl.sampling.sample_neighbors(g, [3, 5, 3], 4, seed=1)
    with pytest.raises(dgl.DGLError, match="repeats a node"):
        dgl.to_block(fr, [3, 5, 3])
    assert _table_is_free()


def _block_arrays(b):
    s, d = _edges_of(b)
    return (s, d, b.srcdata[dgl.NID].cpu().numpy(), b.dstdata[dgl.NID].cpu().numpy(),
            b.number_of_src_nodes(), b.number_of_dst_nodes())


@pytest.mark.parametrize("replace", [False, True])
def test_to_block_fast_path_equals_general_path(replace):
    g, _, (psrc, pdst) = _graph(10, "in")
    seeds = th.tensor([5, 900, 3, 0, 6, 4, 2500, 1], device=DEV)
    fr = dgl.sampling.sample_neighbors(g, seeds, 10, replace=replace, seed=8)
    assert not fr._graph._cache
    fast = dgl.to_block(fr, seeds)
    assert not fr._graph._cache  # the frontier's CSR was never built
    E = fr.number_of_edges()
    assert th.equal(fast.edata[dgl.EID], th.arange(E, device=DEV))
    s, d = fr._graph._device_only
    rebuilt = dgl.DGLGraph.from_device_coo(s, d, N)  # forgets the seeds: the general path
    slow = dgl.to_block(rebuilt, seeds)
    assert rebuilt._graph._cache
    for a, b in zip(_block_arrays(fast), _block_arrays(slow)):
        assert np.array_equal(a, b)
    assert th.equal(fast.edata[dgl.EID], slow.edata[dgl.EID])
    # and against the restatement of the ordering
    fs, fd = _edges_of(fr)
    src_nodes, new_src, uniq = R.relabel(seeds.tolist(), fs.tolist())
    bs, bd, nid_s, nid_d, n_s, n_d = _block_arrays(fast)
    assert np.array_equal(nid_s, src_nodes) and np.array_equal(bs, new_src) and uniq == 8
    assert np.array_equal(nid_d[bd], fd) and n_s == len(src_nodes) and n_d == 8
    assert np.array_equal(nid_s[:n_d], nid_d)  # X[:n_dst] are the destinations' rows
    # other destinations than the seeds: the general path, not the frontier's edge list
    other = dgl.to_block(fr, th.tensor([3, 5], device=DEV))
    assert other.dstdata[dgl.NID].tolist() == [3, 5]
    eid = other.edata[dgl.EID].cpu().numpy()
    assert np.array_equal(fd[eid], np.repeat([3, 5], [np.sum(fd == 3), np.sum(fd == 5)]))
    assert _table_is_free()


def test_to_block_twice_on_different_frontiers():
    g, _, _ = _graph(5, "in")
    for seeds in ([5, 4, 3], [6, 2, 5, 1, 9], [4]):
        fr = dgl.sampling.sample_neighbors(g, seeds, 5, seed=3)
        b = dgl.to_block(fr, seeds)
        fs, fd = _edges_of(fr)
        src_nodes, new_src, _ = R.relabel(seeds, fs.tolist())
        assert np.array_equal(b.srcdata[dgl.NID].cpu().numpy(), src_nodes)
        assert np.array_equal(_edges_of(b)[0], new_src)
        assert _table_is_free()


def test_relabel_kernel_against_the_restatement():
    rng = np.random.default_rng(5)
    for S, E, n in ((0, 0, 10), (1, 0, 10), (0, 7, 10), (300, 5000, 700), (257, 255, 100000)):
        dst = rng.permutation(n)[:S]
        src = rng.integers(0, n, E)
        for include in (True, False):
            args = (th.from_numpy(dst.astype(np.int32)).to(DEV),
                    th.from_numpy(src.astype(np.int32)).to(DEV), n, include)
            got = K.block_relabel(*args)
            again = K.block_relabel(*args)
            assert th.equal(got[0], again[0]) and th.equal(got[1], again[1]) and got[2] == again[2]
            want = R.relabel(dst.tolist(), src.tolist(), include)
            assert np.array_equal(got[0].cpu().numpy(), want[0])
            assert np.array_equal(got[1].cpu().numpy(), want[1]) and got[2] == want[2]
            assert _table_is_free()


# ---- end to end ---------------------------------------------------------------------------
def _block_and_twin(fanout=5):
    g, _, _ = _graph(10, "in")
    seeds = th.tensor([5, 3, 4, 6, 2, 1, 0, 77], device=DEV)
    fr = dgl.sampling.sample_neighbors(g, seeds, fanout, seed=21)
    block = dgl.to_block(fr, seeds)
    s, d = _edges_of(block)
    twin = dgl.bipartite((s, d), num_nodes=(block.number_of_src_nodes(), block.number_of_dst_nodes()))
    return block, twin


@pytest.mark.parametrize("module", ["sage", "gat"])
def test_conv_on_a_block_equals_the_host_bipartite_graph(module):
    block, twin = _block_and_twin()
    th.manual_seed(0)
    conv = (SAGEConv(12, 6, "mean") if module == "sage" else GATConv((12, 12), 6, 3)).to(DEV)
    x = th.randn(block.number_of_src_nodes(), 12, device=DEV)
    outs, grads = [], []
    for g in (block, twin):
        h = x.clone().requires_grad_()
        out = conv(g, (h, h[:g.number_of_dst_nodes()]))
        out.square().sum().backward()
        outs.append(out.detach())
        grads.append(h.grad)
    assert outs[0].shape[0] == block.number_of_dst_nodes()
    assert th.allclose(outs[0], outs[1], **TOL), (outs[0] - outs[1]).abs().max()
    assert th.allclose(grads[0], grads[1], **TOL), (grads[0] - grads[1]).abs().max()
    assert float(outs[0].abs().sum()) > 0


def test_example_runs():
    out = subprocess.check_output(
        [sys.executable, os.path.join(ROOT, "examples", "graphsage_sampling.py")], timeout=300)
    assert b"ok" in out.splitlines()[-1], out[-500:]
