"""dgl.traversal / dgl.propagate on the device against the sequential loops of
traversal_ref.py, run over the project's own CSRs read back to the host.  Every comparison
is integer and exact: ids, order and sections, for every kernel route."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as th

import dgl
import dgl.function as fn
from dgl import kernel as K
from dgl._ffi import DGLError

import traversal_ref as R

pytestmark = pytest.mark.gpu
DEV = th.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HUB = 5000
_G = {}


def _consts():
    t, nl, cap = K.traverse_tile(), K.traverse_narrow_limit(), K.traverse_max_levels_per_launch()
    assert t % 64 == 0 and nl % t == 0
    return t, nl, cap


def _ruler(g):
    """root 0 -> 1, 2, 3, mid, 4, 5 (rows of degree 0 first, last and several in a row around
    mid = 6); mid has g out-edges into the leaves 10 .. 159 with parallel edges, its first and
    its last entry pointing at leaf 159 alone.  Nodes 160, 161 are unreachable."""
    cols = 10 + (7 * np.arange(g)) % 149
    if g >= 2:
        cols[0] = cols[-1] = 159
    return 162, np.r_[np.zeros(6, np.int64), np.full(g, 6)], np.r_[[1, 2, 3, 6, 4, 5], cols], [0]


def _chain(n):
    return n, np.arange(n - 1), np.arange(1, n), [0]


def _broom():
    """chain 0..4 -> a star of 3 NarrowLimit leaves -> one sink -> a chain: narrow, wide, narrow."""
    w = 3 * _consts()[1]
    leaves = 5 + np.arange(w)
    sink = 5 + w
    src = np.r_[np.arange(4), np.full(w, 4), leaves, sink + np.arange(4)]
    dst = np.r_[np.arange(1, 5), leaves, np.full(w, sink), sink + 1 + np.arange(4)]
    return sink + 5, src, dst, [0]


def _layered():
    rng = np.random.default_rng(5)
    layer = np.sort(rng.integers(0, 12, 400))          # a node's layer
    perm = rng.permutation(400)                        # ids do not follow the layers
    u, v = rng.integers(0, 400, 3000), rng.integers(0, 400, 3000)
    keep = layer[u] < layer[v]
    return 400, perm[u[keep]], perm[v[keep]], [int(perm[0]), int(perm[1])]


def _case(name):
    t, nl, cap = _consts()
    sizes = {"G0": 0, "G1": 1, "G63": 63, "G64": 64, "G65": 65, "Gt-1": t - 1, "Gt": t, "Gt+1": t + 1,
             "G2t+1": 2 * t + 1, "Gnl-1": nl - 1, "Gnl": nl, "Gnl+1": nl + 1, "hub": HUB}
    if name in sizes:
        return _ruler(sizes[name])
    if name.startswith("chain"):
        return _chain({"chain300": 300}.get(name) or cap + int(name[5:]))
    return {
        "broom": _broom,
        "layered": _layered,
        # in-edges of node 3 arrive from three levels
        "three_levels": lambda: (4, np.array([0, 1, 0, 1, 2]), np.array([1, 2, 3, 3, 3]), [0]),
        # parallel edges, self loops, duplicate sources (BFS only: it has loops)
        "loops": lambda: (5, np.array([0, 0, 0, 1, 1, 2, 2, 0]), np.array([0, 1, 1, 0, 2, 2, 3, 3]),
                          [0, 1, 0, 0, 1]),
        "cycle": lambda: (4, np.array([0, 1, 2, 3]), np.array([1, 2, 3, 1]), [0]),
        "no_out_edge": lambda: _ruler(65)[:3] + ([159, 20],),
    }[name]()


def _graph(name, bits):
    """(graph, source, {reverse: (walked CSR, opposite indptr)} on the host), built once."""
    if (name, bits) not in _G:
        n, src, dst, source = _case(name)
        g = dgl.DGLGraph()
        g.add_nodes(n)
        g.add_edges(src, dst)
        if bits == 64:
            g._graph = g._graph.asbits(64)
        gidx = g._graph.get_immutable_gidx(DEV)
        assert gidx.out_csr.bits == bits
        host = [tuple(a.cpu().numpy().astype(np.int64) for a in (c.indptr, c.indices, c.data))
                for c in (gidx.out_csr, gidx.in_csr)]
        _G[(name, bits)] = (g, source, {False: (host[0], host[1][0]), True: (host[1], host[0][0])})
    return _G[(name, bits)]


def _lists(frontiers):
    assert all(f.dtype == th.int64 and f.device == DEV for f in frontiers)
    return [f.tolist() for f in frontiers]


DAGS = ["G0", "G1", "G63", "G64", "G65", "Gt-1", "Gt", "Gt+1", "G2t+1", "Gnl-1", "Gnl", "Gnl+1", "hub",
        "chain-1", "chain+0", "chain+1", "chain+2", "chain300", "broom", "layered", "three_levels",
        "no_out_edge"]


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", DAGS + ["loops", "cycle"])
def test_bfs_matches_the_queue(name, bits, reverse):
    g, source, host = _graph(name, bits)
    csr = host[reverse][0]
    if reverse and name.startswith("G"):
        source = [159, 20, 159]  # leaves, one of them twice, back up to the root
    want_n, want_e = R.bfs(csr, source), R.bfs(csr, source, edges=True)
    for variant in (0, 1, 2):  # route identity: every route gives the reference's bits
        assert _lists(dgl.bfs_nodes_generator(g, source, reverse, variant=variant)) == want_n
        assert _lists(dgl.bfs_edges_generator(g, source, reverse, variant=variant)) == want_e
    if name == "hub" and not reverse:  # the contract, spelled out: first occurrence wins
        assert want_n[2][0] == 159 and want_n[2].count(159) == 1


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", DAGS)
def test_topological_matches_the_countdown(name, bits, reverse):
    g, _, host = _graph(name, bits)
    want = R.topological(*host[reverse])
    for variant in (0, 1, 2):
        assert _lists(dgl.topological_nodes_generator(g, reverse, variant=variant)) == want
    if name == "hub" and not reverse:  # the last decrement places the node
        assert want[2][-1] == 159 and want[2].count(159) == 1


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("name", ["cycle", "loops"])
def test_topological_reports_a_loop(name, variant):
    with pytest.raises(DGLError, match="loop"):
        dgl.topological_nodes_generator(_graph(name, 32)[0], variant=variant)


def test_sources_empty_and_as_device_tensors():
    g, _, host = _graph("G65", 32)
    assert dgl.bfs_nodes_generator(g, []) == () and dgl.bfs_edges_generator(g, []) == ()
    want = R.bfs(host[False][0], [6, 0])
    for src in (np.array([6, 0]), th.tensor([6, 0]), th.tensor([6, 0], device=DEV),
                th.tensor([6, 0], device=DEV, dtype=th.int32)):
        assert _lists(dgl.bfs_nodes_generator(g, src)) == want


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("source", [[0, 162], [-1], [3, 2 ** 32], [[0, 1]], [[0, 1], [2, 3]]])
def test_bad_sources_raise(source, on_device):
    source = th.tensor(source, device=DEV) if on_device else np.array(source)
    with pytest.raises(DGLError):
        dgl.bfs_nodes_generator(_graph("G65", 32)[0], source)


def _forest():
    """A batch of random trees, edges child -> parent, with small-integer features."""
    rng = np.random.default_rng(11)
    trees = []
    for n in (1, 2, 7, 30, 64):
        t = dgl.DGLGraph()
        t.add_nodes(n)
        if n > 1:
            t.add_edges(np.arange(1, n), [int(rng.integers(0, c)) for c in range(1, n)])
        trees.append(t)
    g = dgl.batch(trees)
    return g, rng.integers(-4, 5, (g.number_of_nodes(), 3)).astype(np.float32)


def test_prop_nodes_topo_sums_children_bottom_up():
    g, x = _forest()
    g.ndata["h"] = th.from_numpy(x).to(DEV)
    dgl.prop_nodes_topo(g, message_func=fn.copy_u("h", "m"), reduce_func=fn.sum("m", "h"))
    src, dst = (a.numpy() for a in g.all_edges())
    want = x.astype(np.float64)
    for frontier in R.topological(*_host(g))[1:]:
        for v in frontier:  # children are in earlier frontiers: their sums are final
            want[v] = want[src[dst == v]].sum(0)
    assert np.array_equal(g.ndata["h"].cpu().numpy().astype(np.float64), want)


def _host(g):
    gidx = g._graph.get_immutable_gidx(DEV)
    out = tuple(a.cpu().numpy().astype(np.int64)
                for a in (gidx.out_csr.indptr, gidx.out_csr.indices, gidx.out_csr.data))
    return out, gidx.in_csr.indptr.cpu().numpy().astype(np.int64)


def _docstring_graph():
    g = dgl.DGLGraph()
    g.add_nodes(4)
    g.add_edges([0, 1, 1, 2], [1, 2, 3, 3])
    g.ndata["x"] = th.tensor([[1.], [2.], [3.], [4.]], device=DEV)
    return g


def test_prop_nodes_bfs_on_the_docstring_graph():
    g, h = _docstring_graph(), _docstring_graph()
    mr = dict(message_func=fn.copy_u("x", "m"), reduce_func=fn.sum("m", "x"))
    assert _lists(dgl.bfs_nodes_generator(g, 0)) == [[0], [1], [2, 3]]
    dgl.prop_nodes_bfs(g, 0, **mr)
    h.prop_nodes([[0], [1], [2, 3]], **mr)
    assert g.ndata["x"].flatten().tolist() == h.ndata["x"].flatten().tolist() == [1., 1., 1., 4.]


def test_prop_edges_equals_send_and_recv_by_hand():
    g, h = _docstring_graph(), _docstring_graph()
    mr = (fn.copy_u("x", "m"), fn.sum("m", "x"))
    frontiers = dgl.bfs_edges_generator(g, [0])
    assert _lists(frontiers) == [[0], [1, 2]]
    dgl.prop_edges(g, frontiers, *mr)
    for f in frontiers:
        h.send_and_recv(f, *mr)
    assert g.ndata["x"].flatten().tolist() == h.ndata["x"].flatten().tolist()


def test_tree_lstm_example_loss_falls():
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "examples", "tree_lstm.py"),
                                   "--steps", "8"], timeout=300)
    r = json.loads(out.decode().strip().splitlines()[-1])
    assert r["loss_last"] < r["loss_first"], r
