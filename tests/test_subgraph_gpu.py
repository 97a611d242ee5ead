"""DGLGraph.subgraph / edge_subgraph on the device against plain loops: the CSRSliceMatrix
loop over the project's own out-CSR read back to the host, and the first-appearance relabel
loop.  Every comparison is integer and exact."""
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

pytestmark = pytest.mark.gpu
DEV = th.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = None  # DGLMISubgraphTile(), read on first use
HUB = 5000
# nodes 0 .. 199 have no out-edge; 0 .. 149 are the only columns of the ruler rows
ZERO, COLS, NOCOL = 200, 150, np.arange(150, 200)
_G = {}


def _tile():
    global T
    if T is None:
        T = K.subgraph_tile()
        assert T % 64 == 0
    return T


def _graph(bits):
    """Ruler rows of degree 1, 63, 64, 65, T - 1, T, T + 1, 2T + 1 and HUB (row r of degree g:
    columns 7k mod 150, so parallel edges abound), a row of self loops and parallel edges,
    and a row W of degree T whose first word points at node 160, last word at 161 and the
    rest at 162.  Returns (graph, {degree: row}, loop row, W, host out-CSR)."""
    if bits not in _G:
        t = _tile()
        degs = [1, 63, 64, 65, t - 1, t, t + 1, 2 * t + 1, HUB]
        row_of = {g: ZERO + i for i, g in enumerate(degs)}
        loop, w = ZERO + len(degs), ZERO + len(degs) + 1
        src = [np.full(g, r) for g, r in row_of.items()]
        dst = [(7 * np.arange(g)) % COLS for g in degs]
        src += [np.full(5, loop)]
        dst += [np.array([loop, 3, loop, 3, 3])]
        src, dst = np.concatenate(src), np.concatenate(dst)
        order = np.random.default_rng(7).permutation(len(src))  # CSR data is not the identity
        # row W is added last and in order: a row of the out-CSR keeps insertion order
        w_dst = np.where(np.arange(t) < 64, 160, np.where(np.arange(t) >= t - 64, 161, 162))
        g = dgl.DGLGraph()
        g.add_nodes(w + 1)
        g.add_edges(np.r_[src[order], np.full(t, w)], np.r_[dst[order], w_dst])
        if bits == 64:
            g._graph = g._graph.asbits(64)
        c = g._graph.get_immutable_gidx(DEV).out_csr
        assert c.bits == bits
        host = tuple(a.cpu().numpy().astype(np.int64) for a in (c.indptr, c.indices, c.data))
        _G[bits] = (g, row_of, loop, w, host)
    return _G[bits]


def _ref_slice(host, nodes):
    indptr, indices, data = host
    pos = {int(v): i for i, v in enumerate(nodes)}
    s, d, e = [], [], []
    for i, v in enumerate(nodes):
        for k in range(indptr[v], indptr[v + 1]):
            j = pos.get(int(indices[k]))
            if j is not None:
                s.append(i), d.append(j), e.append(int(data[k]))
    return [th.tensor(x, dtype=th.int64) for x in (s, d, e)]


def _edges(sg):
    s, d = sg.all_edges()
    return s, d, sg.parent_eid.cpu()


def _gval(case):
    """The number of gathered positions a G case is built to have."""
    t = _tile()
    return {"G0": 0, "G1": 1, "G63": 63, "G64": 64, "G65": 65, "Gt-1": t - 1, "Gt": t,
            "Gt+1": t + 1, "G2t+1": 2 * t + 1, "empty": 0}.get(case)


def _nodes(case, r):
    """The node list of a case; ``r``: degree -> ruler row."""
    t = _tile()
    n = ZERO + 11
    z = np.arange(ZERO)
    if case == "G0":
        return z[10:90]
    if case.startswith("G"):  # rows of degree 0 first, last and several in a row
        return np.r_[z[4::-1], r[_gval(case)], z[5:60]]
    return {
        "hub_first": lambda: np.r_[r[HUB], r[65], z[:COLS], r[t + 1]],
        "hub_middle": lambda: np.r_[r[65], z[:70], r[HUB], z[70:COLS], r[t + 1]],
        "hub_last": lambda: np.r_[z[:COLS][::-1], r[65], r[t + 1], r[HUB]],
        "none_kept": lambda: np.r_[NOCOL[:3], r[t + 1], r[64], NOCOL[3:9]],
        "all_permuted": lambda: np.random.default_rng(3).permutation(n),
        "all_ascending": lambda: np.arange(n),
        "all_descending": lambda: np.arange(n)[::-1].copy(),
        "first_word_only": lambda: np.array([n - 1, 160]),
        "last_word_only": lambda: np.array([161, n - 1]),
        "loops_parallel": lambda: np.array([3, n - 2]),
        "empty": lambda: np.empty(0, np.int64),
    }[case]().astype(np.int64)


CASES = ["G0", "G1", "G63", "G64", "G65", "Gt-1", "Gt", "Gt+1", "G2t+1", "hub_first", "hub_middle",
         "hub_last", "none_kept", "all_permuted", "all_ascending", "all_descending",
         "first_word_only", "last_word_only", "loops_parallel", "empty"]


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("case", CASES)
def test_subgraph_equals_slice_loop(case, bits):
    g, row_of, _, _, host = _graph(bits)
    nodes = _nodes(case, row_of)
    if _gval(case) is not None:
        assert int((host[0][nodes + 1] - host[0][nodes]).sum()) == _gval(case)
    ref = _ref_slice(host, nodes)
    if case == "none_kept":
        assert ref[0].numel() == 0
    if case in ("first_word_only", "last_word_only"):
        # row W fills one tile (the other row is empty); its kept positions are one whole word
        t, w = _tile(), nodes.max()
        assert host[0][w + 1] - host[0][w] == t
        kept = np.nonzero(np.isin(host[1][host[0][w]:host[0][w + 1]], nodes))[0]
        first = case == "first_word_only"
        assert np.array_equal(kept, np.arange(0, 64) if first else np.arange(t - 64, t))
    sg = g.subgraph(nodes)
    assert sg.is_readonly and sg.parent is g and sg.number_of_nodes() == len(nodes)
    assert th.equal(sg.parent_nid.cpu(), th.from_numpy(nodes)) and sg.parent_nid.device == DEV
    got = _edges(sg)
    assert all(th.equal(a, b) for a, b in zip(got, ref)), [x.shape for x in got + tuple(ref)]


@pytest.mark.parametrize("dtype", [th.int32, th.int64])
@pytest.mark.parametrize("where", ["host", "device", "numpy", "list"])
def test_subgraph_node_containers(where, dtype):
    g, row_of, _, _, host = _graph(32)
    nodes = _nodes("hub_middle", row_of)
    ref = _ref_slice(host, nodes)
    t = th.from_numpy(nodes).to(dtype)
    arg = {"host": t, "device": t.to(DEV), "numpy": t.numpy(), "list": nodes.tolist()}[where]
    assert all(th.equal(a, b) for a, b in zip(_edges(g.subgraph(arg)), ref))
    a, b = g.subgraphs([arg, nodes[:40]])
    assert th.equal(_edges(a)[2], ref[2]) and b.number_of_nodes() == 40


def _cycle():
    g = dgl.DGLGraph()
    g.add_nodes(5)
    g.add_edges([0, 1, 2, 3, 4], [1, 2, 3, 4, 0])
    return g


def _lists(sg):
    return [x.tolist() for x in _edges(sg)] + [sg.parent_nid.tolist()]


def test_docstring_answers_and_table_restored():
    g = _cycle()
    assert _lists(g.subgraph([0, 1, 4])) == [[0, 2], [1, 0], [0, 4], [0, 1, 4]]
    # the relabel table is clean again: a stale mark on node 0 would change this block
    block = dgl.to_block(g, th.tensor([2, 1], device=DEV))
    assert block.srcdata[dgl.NID].tolist() == [2, 1, 0]
    with pytest.raises(DGLError, match="repeats a node"):
        g.subgraph([0, 1, 0])
    block = dgl.to_block(g, th.tensor([2, 1], device=DEV))
    assert block.srcdata[dgl.NID].tolist() == [2, 1, 0]
    # edges 0 -> 1 and 4 -> 0: sources first (0, 4), then the new destination (1)
    assert _lists(g.edge_subgraph([0, 4])) == [[0, 1], [2, 0], [0, 4], [0, 4, 1]]
    sg = g.edge_subgraph(th.tensor([0, 4], device=DEV), preserve_nodes=True)
    assert _lists(sg) == [[0, 4], [1, 0], [0, 4], [0, 1, 2, 3, 4]]


@pytest.mark.parametrize("bits", [32, 64])
def test_edge_subgraph_equals_first_appearance_loop(bits):
    g, _, _, _, _ = _graph(bits)
    src, dst, _ = g._graph.edges()
    e = np.random.default_rng(5).permutation(g.number_of_edges())[:3000]
    e[7] = e[3]  # an edge may be asked for twice
    new = {}
    for v in np.r_[src[e], dst[e]]:
        new.setdefault(int(v), len(new))
    ref = [[new[int(v)] for v in src[e]], [new[int(v)] for v in dst[e]], e.tolist(), list(new)]
    assert _lists(g.edge_subgraph(e)) == ref
    assert _lists(g.edge_subgraph(th.from_numpy(e).to(DEV).int())) == ref


def test_bookkeeping_and_message_passing():
    g, row_of, _, _, host = _graph(32)
    g = g.local_var()
    n, m = g.number_of_nodes(), g.number_of_edges()
    g.ndata["x"] = th.randint(-8, 8, (n, 3), device=DEV).float()
    g.edata["w"] = th.randint(-8, 8, (m, 2), device=DEV).float()
    g.ndata["k"] = th.arange(n, device=DEV)
    nodes = _nodes("hub_middle", row_of)
    sg = g.subgraph(nodes)
    sg.copy_from_parent()
    nid, eid = sg.parent_nid, sg.parent_eid
    assert th.equal(sg.ndata["x"], g.ndata["x"][nid]) and th.equal(sg.ndata["k"], nid)
    assert th.equal(sg.edata["w"], g.edata["w"][eid])
    perm = th.randperm(len(nodes), device=DEV)
    assert th.equal(sg.map_to_subgraph_nid(nid[perm]), perm)
    with pytest.raises(DGLError, match="not in the subgraph"):
        sg.map_to_subgraph_nid([int(NOCOL[-1])])

    s, d, _ = _ref_slice(host, nodes)
    sg.update_all(fn.copy_u("x", "m"), fn.sum("m", "y"))
    want = th.zeros(len(nodes), 3, device=DEV).index_add_(0, d.to(DEV), sg.ndata["x"][s.to(DEV)])
    assert th.equal(sg.ndata["y"], want)

    before_x, before_w = g.ndata["x"].clone(), g.edata["w"].clone()
    sg.ndata["x"] = sg.ndata["x"] + 100
    sg.edata["w"] = sg.edata["w"] - 100
    sg.copy_to_parent()
    before_x[nid] += 100
    before_w[eid] -= 100
    assert th.equal(g.ndata["x"], before_x) and th.equal(g.edata["w"], before_w)
    assert th.equal(g.ndata["y"][nid], want) and dgl.NID not in g.ndata


def test_errors_are_python_errors():
    g = _cycle()
    with pytest.raises(DGLError, match="out of range"):
        g.subgraph([0, 5])
    with pytest.raises(DGLError, match="out of range"):
        g.subgraph(th.tensor([0, 5], device=DEV))
    wraps = th.tensor([0, 2 ** 32 + 1], device=DEV)  # 1 once narrowed to int32
    with pytest.raises(DGLError, match="out of range"):
        g.subgraph(wraps)
    with pytest.raises(DGLError, match="not in the subgraph"):
        g.subgraph([0, 1]).map_to_subgraph_nid(wraps)
    for bad in ([0, 5], th.tensor([-1, 2], device=DEV)):
        for keep in (False, True):
            with pytest.raises(DGLError, match="out of range"):
                g.edge_subgraph(bad, preserve_nodes=keep)
    th.cuda.synchronize()
    assert _lists(g.subgraph([4, 3]))[:3] == [[1], [0], [3]]  # the device is still healthy


def test_cluster_gcn_example():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cluster_gcn.py")],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cluster_gcn ok" in out.stdout
