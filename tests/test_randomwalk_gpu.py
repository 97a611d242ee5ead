"""Device random walks on the GPU, bit for bit against ``randomwalk_ref.py``, a numpy
restatement of include/dglmi.h.

The homogeneous graph has rows of degree 0, 1, 2 and 5,000 and background rows that lead
into the degree-0 rows, so walks meet dead ends at their first step and in their middle; it
is built by ``add_edges`` in shuffled order.  Walk counts sit on either side of one and of
four wavefronts; lengths are 0, 1, 2, 7 and those whose row length L + 1 sits on either side
of one and of two staging chunks (``dgl.kernel.walk_stage_chunk()`` columns).  Both store
variants and both index widths are compared with one restatement result per shape."""
import os
import sys

import numpy as np
import pytest
import torch as th

import dgl
from dgl import kernel as K

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import randomwalk_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = th.device("cuda:0")
HUB = 5000
N = 5100
WALKS = [1, 63, 64, 65, 255, 256, 257]
_CACHE = {}


def _lengths():
    c = K.walk_stage_chunk()
    return sorted({0, 1, 2, 7, c - 2, c - 1, c, 2 * c - 2, 2 * c - 1, 2 * c})


def _graph(bits=32):
    """Rows 0 .. 3: degree 0, 1 (into row 0), 2, HUB.  Returns (DGLGraph, host out-CSR)."""
    if ("g", bits) not in _CACHE:
        rng = np.random.default_rng(2026)
        rows = [np.full(1, 1), np.full(2, 2), np.full(HUB, 3)]
        cols = [np.array([0]), np.array([1, 3]), rng.choice(N, HUB, replace=False)]
        rows.append(rng.integers(4, N, 6000))   # background: some rows stay empty, and
        cols.append(rng.integers(0, N, 6000))   # some edges lead into rows 0 .. 3
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        order = rng.permutation(len(rows))
        g = dgl.DGLGraph()
        g.add_nodes(N)
        g.add_edges(rows[order], cols[order])
        if bits == 64:
            g._graph = g._graph.asbits(64)
        (indptr, indices, _), _ = g._graph.host_csr()
        deg = np.diff(indptr)
        assert deg[:4].tolist() == [0, 1, 2, HUB] and (deg[4:] == 0).any()
        _CACHE[("g", bits)] = (g, (np.asarray(indptr), np.asarray(indices)))
    return _CACHE[("g", bits)]


def _csr(g):
    return g._graph.get_immutable_gidx(DEV).out_csr


def _seeds(n):
    rng = np.random.default_rng(n)
    s = np.concatenate([np.resize(np.array([3, 2, 1, 0, 3, 3]), n)[: n // 2],
                        rng.integers(0, N, n - n // 2)])
    return s[:n]


def _t32(a):
    return th.from_numpy(np.asarray(a).astype(np.int32)).to(DEV)


def _thr(values):
    return None if values is None else th.tensor(list(values), dtype=th.int64).to(DEV)


def _want(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("n", WALKS)
def test_walks_match_the_restatement(n, bits):
    g, host = _graph(bits)
    csr = _csr(g)
    assert csr.bits == bits
    seeds = _seeds(n)
    for L in _lengths():
        rng_seed = 0x9E3779B97F4A7C15 + 1000 * n + L
        for name, thr in (("none", None), ("half", [R.threshold(0.5)] * L)):
            want = _want(("w", n, L, name),
                         lambda: R.walk([host], [0] * L, seeds, thr, rng_seed))
            path = _t32([0] * L)
            for variant in (0, 1, 2):
                got = K.random_walk([csr], path, _t32(seeds), _thr(thr), rng_seed, variant=variant)
                assert got.dtype == th.int64 and tuple(got.shape) == (n, L + 1)
                assert np.array_equal(got.cpu().numpy(), want), (n, L, name, variant, bits)


def test_the_graph_exercises_dead_ends_and_the_hub():
    _, host = _graph()
    tr = R.walk([host], [0] * 7, _seeds(257), None, 5)
    ends = (tr >= 0).sum(1)
    assert (ends == 1).any() and ((ends > 2) & (ends < 8)).any() and (ends == 8).any()
    assert (tr[:, 0] == 3).any() and (tr[:, 0] == 0).any()


def test_device_seeds_outside_the_graph_and_repeats():
    g, host = _graph()
    seeds = np.array([3, N, -1, 3, 2 ** 31 - 1, 3, 2, 2, -7, N + 5])
    got = K.random_walk([_csr(g)], _t32([0] * 3), _t32(seeds), None, 11)
    want = R.walk([host], [0] * 3, seeds, None, 11)
    assert np.array_equal(got.cpu().numpy(), want)
    out = got.cpu().numpy()
    for row in (1, 2, 4, 8, 9):
        assert out[row, 1:].tolist() == [-1, -1, -1] and out[row, 0] == seeds[row]
    assert not np.array_equal(out[0], out[3])  # equal seeds, different slots: different draws


def test_restarts_with_known_columns():
    """Restart 0 never stops, 1 always stops after the first step, and a stepwise vector of
    zeros and ones stops at its first one: on a self-loop the last column is known exactly."""
    g = dgl.DGLGraph()
    g.add_nodes(2)
    g.add_edges([0, 0, 0], [0, 0, 0])
    csr, L, n = _csr(g), 9, 130
    path, seeds = _t32([0] * L), _t32([0] * n)
    host = (np.array([0, 3, 3]), np.array([0, 0, 0]))

    def run(probs):
        thr = K.restart_thresholds(probs)
        got = K.random_walk([csr], path, seeds, _thr(thr), 77).cpu().numpy()
        assert np.array_equal(got, R.walk([host], [0] * L, [0] * n, thr, 77))
        return got

    assert (run([0.0] * L) == 0).all()
    assert (run([2.0 ** -33] * L) == 0).all()
    for p in (1.0, 1.5):
        one = run([p] * L)
        assert (one[:, :2] == 0).all() and (one[:, 2:] == -1).all()
    step = run([0, 0, 0, 1, 0, 1, 0, 0, 0])
    assert (step[:, :5] == 0).all() and (step[:, 5:] == -1).all()
    half = run([0.5] * L)
    lengths = (half >= 0).sum(1)
    assert lengths.min() >= 2 and len(set(lengths.tolist())) > 3


def _hetero():
    """user (40) -follow-> user, user -view-> item (25), item -viewed-by-> user; some users
    view nothing and some items are viewed by nobody."""
    if "h" not in _CACHE:
        rng = np.random.default_rng(8)
        nu, ni = 40, 25
        fol = (rng.integers(0, nu, 90), rng.integers(0, nu, 90))
        view = (rng.integers(0, nu - 6, 70), rng.integers(0, ni, 70))
        by = (rng.integers(0, ni - 4, 60), rng.integers(0, nu, 60))
        g = dgl.heterograph({("user", "follow", "user"): fol, ("user", "view", "item"): view,
                             ("item", "viewed-by", "user"): by},
                            num_nodes_dict={"user": nu, "item": ni})

        def csr(uv, n):
            order = np.argsort(uv[0], kind="stable")
            indptr = np.concatenate([[0], np.cumsum(np.bincount(uv[0], minlength=n))])
            return indptr, uv[1][order]
        _CACHE["h"] = (g, {"follow": csr(fol, nu), "view": csr(view, nu), "viewed-by": csr(by, ni)})
    return _CACHE["h"]


def test_metapath_across_two_node_types():
    g, host = _hetero()
    assert g.ntypes == ["user", "item"]
    metapath = ["follow", "view", "viewed-by"] * 2 + ["view"]
    seeds = np.arange(40).repeat(3)
    traces, types = dgl.sampling.random_walk(g, seeds, metapath=metapath, seed=123)
    assert types.tolist() == [0, 0, 1, 0, 0, 1, 0, 1] and types.dtype == th.int64
    assert traces.device.type == "cuda" and types.device.type == "cuda"
    rels = [host["follow"], host["view"], host["viewed-by"]]  # order of first use
    want = R.walk(rels, [0, 1, 2, 0, 1, 2, 1], seeds, None, 123)
    assert np.array_equal(traces.cpu().numpy(), want)
    assert (want[:, -1] >= 0).any() and (want[:, 2] == -1).any()
    # a metapath that starts with another relation: the table's order follows it
    traces, types = dgl.sampling.random_walk(
        g, th.arange(25).to(DEV), metapath=["viewed-by", ("user", "view", "item")],
        restart_prob=th.tensor([0.0, 0.5]), seed=5)
    assert types.tolist() == [1, 0, 1]
    want = R.walk([host["viewed-by"], host["view"]], [0, 1], np.arange(25),
                  [0, R.threshold(0.5)], 5)
    assert np.array_equal(traces.cpu().numpy(), want)


def test_counter_same_seed_and_torch_seed():
    g, host = _graph()
    csr, seeds = _csr(g), _seeds(70)
    path = _t32([0] * 5)
    for ctr in (1, 2 ** 32 - 1, 2 ** 64 - 3):
        got = K.random_walk([csr], path, _t32(seeds), None, 3, rng_ctr=ctr)
        assert np.array_equal(got.cpu().numpy(), R.walk([host], [0] * 5, seeds, None, 3, rng_ctr=ctr))
    a, types = dgl.sampling.random_walk(g, seeds, length=5, seed=99)
    b, _ = dgl.sampling.random_walk(g, th.from_numpy(seeds).to(DEV), length=5, seed=99)
    assert th.equal(a, b) and types.tolist() == [0] * 6
    assert np.array_equal(a.cpu().numpy(), R.walk([host], [0] * 5, seeds, None, 99))
    c, _ = dgl.sampling.random_walk(g, seeds, length=5, seed=100)
    assert not th.equal(a, c)
    th.manual_seed(4)
    d, _ = dgl.sampling.random_walk(g, seeds, length=5, restart_prob=0.25)
    e, _ = dgl.sampling.random_walk(g, seeds, length=5, restart_prob=0.25)
    th.manual_seed(4)
    f, _ = dgl.sampling.random_walk(g, seeds, length=5, restart_prob=0.25)
    assert th.equal(d, f) and not th.equal(d, e)
    th.manual_seed(4)
    drawn = int(th.randint(0, 2 ** 63 - 1, (1,), dtype=th.int64).item())
    want = R.walk([host], [0] * 5, seeds, [R.threshold(0.25)] * 5, drawn)
    assert np.array_equal(d.cpu().numpy(), want)


def test_single_relation_heterograph_and_no_walks():
    g = dgl.graph(([0, 1, 2], [1, 2, 0]), "user", "follows")
    traces, types = dgl.sampling.random_walk(g, [0, 1], length=4, seed=1)
    assert traces.tolist() == [[0, 1, 2, 0, 1], [1, 2, 0, 1, 2]] and types.tolist() == [0] * 5
    traces, types = dgl.sampling.random_walk(g, [], length=4, seed=1)
    assert tuple(traces.shape) == (0, 5) and types.tolist() == [0] * 5
    traces, _ = dgl.sampling.random_walk(g, [2, 2], length=0, seed=1)
    assert traces.tolist() == [[2], [2]]


def test_c_entry_rejects_bad_arguments():
    g, _ = _graph()
    csr = _csr(g)
    with pytest.raises(dgl.DGLError, match="between 1 and %d" % K.walk_max_relations()):
        K.random_walk([csr] * (K.walk_max_relations() + 1), _t32([0]), _t32([0]), None, 1)
    with pytest.raises(dgl.DGLError, match="variant must be 0, 1 or 2"):
        K.random_walk([csr], _t32([0]), _t32([0]), None, 1, variant=3)
    with pytest.raises(dgl.DGLError, match="thresholds"):
        K.random_walk([csr], _t32([0, 0]), _t32([0]), _thr([1]), 1)


def test_pack_traces():
    g, _ = _graph()
    traces, types = dgl.sampling.random_walk(g, _seeds(90), length=6, restart_prob=0.3, seed=8)
    traces = th.cat([traces, th.full((1, 7), -1, dtype=th.int64, device=DEV)])  # all padding
    types = th.tensor([0, 1, 0, 1, 0, 1, 0], device=DEV)
    vids, vtypes, lengths, offsets = dgl.sampling.pack_traces(traces, types)
    tr = traces.cpu().numpy()
    want_v, want_t, want_l, want_o = [], [], [], []
    for row in tr:
        want_o.append(len(want_v))
        keep = [j for j, v in enumerate(row) if v != -1]
        want_v.extend(row[keep])
        want_t.extend(types.cpu().numpy()[keep])
        want_l.append(len(keep))
    assert vids.tolist() == [int(v) for v in want_v] and vtypes.tolist() == [int(t) for t in want_t]
    assert lengths.tolist() == want_l and offsets.tolist() == want_o
    assert want_l[-1] == 0 and min(want_l[:-1]) >= 1 and vids.device.type == "cuda"
