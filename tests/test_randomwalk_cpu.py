"""Random walks and the PinSAGE samplers without a GPU: the names, every host-side validation
error of ``dgl.sampling.random_walk`` / ``RandomWalkNeighborSampler`` / ``PinSAGESampler``
(raised before any launch, so host graphs and host ids reach them), the restart threshold
rule, the draw layout, and the statistics of the contract's algorithm, checked on the numpy
restatement (``randomwalk_ref.py``) alone.

Statistics.  Pearson's statistic is compared with the 1 - 1e-6 quantile of chi-square with
(bins - 1) degrees of freedom, ``test_sampling_cpu.py``'s bound.  The RNG seeds are named
below (SEEDS); the restatement passes with each of them."""
import os
import sys

import numpy as np
import pytest
import torch as th

import dgl
from dgl import kernel as K

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import randomwalk_ref as R  # noqa: E402
from sampling_ref import philox4x32_10  # noqa: E402
from test_sampling_cpu import _chi2_quantile  # noqa: E402

SEEDS = (20261021, 7, 0x5EED5EED5EED)


def test_names_are_importable():
    from dgl.sampling import PinSAGESampler, RandomWalkNeighborSampler, pack_traces, random_walk
    assert dgl.sampling.random_walk is random_walk and dgl.sampling.pack_traces is pack_traces
    assert issubclass(PinSAGESampler, RandomWalkNeighborSampler)
    for name in ("random_walk", "visit_topk", "visit_tile", "walk_max_relations", "visit_max_k",
                 "visit_max_width"):
        assert callable(getattr(K, name))
    assert K.walk_max_relations() >= 8
    assert K.visit_max_k() >= 64 and K.visit_max_width() >= 4096
    padded, per_wg = K.visit_tile(1, 1)
    assert padded >= 1 and per_wg >= 1
    with pytest.raises(dgl.DGLError, match="between 1 and %d" % K.visit_max_width()):
        K.visit_tile(K.visit_max_width() + 1, 1)
    with pytest.raises(dgl.DGLError, match="K must be between 1 and %d" % K.visit_max_k()):
        K.visit_tile(8, K.visit_max_k() + 1)


def _g():
    g = dgl.DGLGraph()
    g.add_nodes(6)
    g.add_edges([0, 1, 2, 3, 4], [1, 2, 3, 4, 5])
    return g


def _hg():
    return dgl.heterograph({
        ("user", "follow", "user"): ([0, 1, 1, 2, 3], [1, 2, 3, 0, 0]),
        ("user", "view", "item"): ([0, 0, 1, 2, 3, 3], [0, 1, 1, 2, 2, 1]),
        ("item", "viewed-by", "user"): ([0, 1, 1, 2, 2, 1], [0, 0, 1, 2, 3, 3])},
        num_nodes_dict={"user": 4, "item": 3})


@pytest.fixture
def no_launch(monkeypatch):
    """Fail the test if anything reaches the library's launching entries."""
    def boom(*a, **k):
        raise AssertionError("a launch was attempted before validation finished")
    for name in ("random_walk", "visit_topk"):
        monkeypatch.setattr(K, name, boom)


def test_prob_is_not_built(no_launch):
    with pytest.raises(dgl.DGLError, match="weighted walks are not built"):
        dgl.sampling.random_walk(_g(), [1], length=2, prob="p")


def test_neither_metapath_nor_length(no_launch):
    with pytest.raises(dgl.DGLError, match="either metapath or length"):
        dgl.sampling.random_walk(_g(), [1])
    with pytest.raises(dgl.DGLError, match="either metapath or length"):
        dgl.sampling.random_walk(dgl.graph(([0], [1])), [0])
    with pytest.raises(dgl.DGLError, match="give metapath, not length"):
        dgl.sampling.random_walk(_hg(), [0], length=2)


@pytest.mark.parametrize("length", [2.0, "3", True, float("nan")])
def test_length_must_be_an_int(no_launch, length):
    with pytest.raises(dgl.DGLError, match="length must be an int"):
        dgl.sampling.random_walk(_g(), [1], length=length)


def test_negative_length(no_launch):
    with pytest.raises(dgl.DGLError, match="length must not be negative"):
        dgl.sampling.random_walk(_g(), [1], length=-1)


@pytest.mark.parametrize("seed", [1.5, "7", True, -1, float("nan")])
def test_bad_seed(no_launch, seed):
    with pytest.raises(dgl.DGLError, match="seed must be a non-negative int"):
        dgl.sampling.random_walk(_g(), [1], length=2, seed=seed)


@pytest.mark.parametrize("p", [-0.1, float("nan"), "0.5", True, object()])
def test_bad_scalar_restart_prob(no_launch, p):
    with pytest.raises(dgl.DGLError, match="restart_prob"):
        dgl.sampling.random_walk(_g(), [1], length=2, restart_prob=p)


@pytest.mark.parametrize("p", [th.tensor([0.5, -1.0]), th.tensor([0.5, float("nan")]),
                               np.array([0.1, -0.0001]), ["a", "b"]])
def test_bad_restart_prob_entry(no_launch, p):
    with pytest.raises(dgl.DGLError, match="restart_prob"):
        dgl.sampling.random_walk(_g(), [1], length=2, restart_prob=p)


@pytest.mark.parametrize("p", [th.tensor([0.5]), th.tensor([0.1, 0.2, 0.3]), th.zeros(2, 1),
                               np.zeros(0)])
def test_restart_prob_of_the_wrong_length(no_launch, p):
    with pytest.raises(dgl.DGLError, match="one value per step"):
        dgl.sampling.random_walk(_g(), [1], length=2, restart_prob=p)


def test_unknown_edge_type(no_launch):
    with pytest.raises(dgl.DGLError, match="unknown edge type 'likes'"):
        dgl.sampling.random_walk(_hg(), [0], metapath=["follow", "likes"])
    with pytest.raises(dgl.DGLError, match="unknown edge type"):
        dgl.sampling.random_walk(_hg(), [0], metapath=[("user", "follow", "item")])
    with pytest.raises(dgl.DGLError, match="must be a list"):
        dgl.sampling.random_walk(_hg(), [0], metapath="follow")
    with pytest.raises(dgl.DGLError, match="no edge types"):
        dgl.sampling.random_walk(_g(), [0], metapath=["follow"])


def test_metapath_that_does_not_chain(no_launch):
    with pytest.raises(dgl.DGLError, match="does not chain at step 1"):
        dgl.sampling.random_walk(_hg(), [0], metapath=["view", "follow"])
    with pytest.raises(dgl.DGLError, match="does not chain at step 2"):
        dgl.sampling.random_walk(_hg(), [0], metapath=["follow", "view", "view"])
    b = dgl.bipartite(([0, 1], [0, 0]), num_nodes=(2, 1))
    with pytest.raises(dgl.DGLError, match="does not chain"):
        dgl.sampling.random_walk(b, [0], length=2)


@pytest.mark.parametrize("nodes", [[6], [-1], [0, 1, 99], th.tensor([2, 6]), np.array([-3])])
def test_host_seed_out_of_range(no_launch, nodes):
    with pytest.raises(dgl.DGLError, match="out of range"):
        dgl.sampling.random_walk(_g(), nodes, length=2)


def test_host_seed_range_is_the_first_source_type(no_launch):
    with pytest.raises(dgl.DGLError, match=r"out of range \[0, 3\)"):
        dgl.sampling.random_walk(_hg(), [3], metapath=["viewed-by", "view"])
    with pytest.raises(dgl.DGLError, match=r"out of range \[0, 4\)"):
        dgl.sampling.random_walk(_hg(), [4], metapath=["view", "viewed-by"])


def test_float_ids(no_launch):
    with pytest.raises(dgl.DGLError, match="must hold integers"):
        dgl.sampling.random_walk(_g(), th.tensor([1.0]), length=2)


def test_too_many_relations(no_launch):
    n = K.walk_max_relations() + 1
    g = dgl.heterograph({("a", "e%d" % i, "a"): ([0], [0]) for i in range(n)})
    with pytest.raises(dgl.DGLError, match="limit of %d" % K.walk_max_relations()):
        dgl.sampling.random_walk(g, [0], metapath=["e%d" % i for i in range(n)])


def test_not_a_graph(no_launch):
    with pytest.raises(dgl.DGLError, match="DGLGraph or a DGLHeteroGraph"):
        dgl.sampling.random_walk("graph", [0], length=1)


def test_no_device(no_launch, monkeypatch):
    monkeypatch.setattr(th.cuda, "is_available", lambda: False)
    with pytest.raises(dgl.DGLError, match="ROCm devices only"):
        dgl.sampling.random_walk(_g(), [1], length=2)
    with pytest.raises(dgl.DGLError, match="ROCm devices only"):
        dgl.sampling.random_walk(_hg(), [1], metapath=["follow"])
    with pytest.raises(dgl.DGLError, match="ROCm devices only"):
        dgl.sampling.RandomWalkNeighborSampler(_g(), 2, 0.5, 4, 3)([0])


def test_sampler_limits_name_the_limit(no_launch):
    S = dgl.sampling.RandomWalkNeighborSampler
    with pytest.raises(dgl.DGLError, match="num_neighbors = %d is above the kernel's limit of %d"
                       % (K.visit_max_k() + 1, K.visit_max_k())):
        S(_g(), 2, 0.5, 4, K.visit_max_k() + 1)
    w = K.visit_max_width()
    with pytest.raises(dgl.DGLError, match="= %d is above the kernel's limit of %d" % (w + 2, w)):
        S(_g(), 2, 0.5, w // 2 + 1, 3)
    with pytest.raises(dgl.DGLError, match="at least 1"):
        S(_g(), 0, 0.5, 4, 3)
    with pytest.raises(dgl.DGLError, match="num_neighbors must be an int"):
        S(_g(), 2, 0.5, 4, 3.0)
    with pytest.raises(dgl.DGLError, match="restart_prob"):
        S(_g(), 2, -0.5, 4, 3)
    with pytest.raises(dgl.DGLError, match="seed must be"):
        S(_g(), 2, 0.5, 4, 3, seed=0.5)


def test_sampler_metapath_errors(no_launch):
    S = dgl.sampling.RandomWalkNeighborSampler
    with pytest.raises(dgl.DGLError, match="metapath must be given"):
        S(_hg(), 2, 0.5, 4, 3)
    with pytest.raises(dgl.DGLError, match="start and end at the same node type"):
        S(_hg(), 1, 0.5, 4, 3, metapath=["follow", "view"])
    with pytest.raises(dgl.DGLError, match="unknown edge type"):
        S(_hg(), 1, 0.5, 4, 3, metapath=["likes"])
    with pytest.raises(dgl.DGLError, match="no edge type from 'item' to 'item'"):
        dgl.sampling.PinSAGESampler(_hg(), "item", "item", 2, 0.5, 4, 3)
    s = dgl.sampling.PinSAGESampler(_hg(), "item", "user", 2, 0.5, 4, 3)
    assert s.ntype == "item" and s.metapath_hops == 2
    assert s.restart_prob == [0.0, 0.0, 0.5, 0.0]
    with pytest.raises(dgl.DGLError, match=r"out of range \[0, 3\)"):
        s([3])


# ---- the restatement itself ----------------------------------------------------------
def test_restart_threshold_rule():
    assert R.threshold(0.0) == 0
    assert R.threshold(2.0 ** -33) == 0          # below the quantum: never stops
    assert R.threshold(0.5) == 2 ** 31
    assert R.threshold(1.0) == 2 ** 32           # above every 32-bit draw: always stops
    assert R.threshold(1.5) == 2 ** 32
    ps = [0.0, 2.0 ** -33, 0.5, 1.0, 1.5, 0.3]
    assert K.restart_thresholds(ps) == [R.threshold(p) for p in ps]
    # a draw y stops the walk iff y < threshold: exactly threshold of the 2^32 values
    for y, thr, stops in ((0, 0, False), (0, 1, True), (2 ** 32 - 1, 2 ** 32, True),
                          (2 ** 31, 2 ** 31, False), (2 ** 31 - 1, 2 ** 31, True)):
        assert (y < thr) is stops


def test_draw_layout():
    """Step t of walk i: the block at counter rng_ctr + t, slot i; x picks, y restarts."""
    seed, ctr = 0x1234567890ABCDEF, 2 ** 32 - 1
    x, y = R.walk_draws(seed, ctr, 4, 5)
    for i in range(4):
        for t in range(5):
            c = ctr + t
            blk = philox4x32_10(c & 0xFFFFFFFF, c >> 32, i, 0, 0x90ABCDEF, 0x12345678)
            assert int(x[i, t]) == int(blk[0]) and int(y[i, t]) == int(blk[1])
    # which component feeds which decision: a star whose hub row is 0 .. 2^16 - 1
    deg = 2 ** 16
    csr = (np.array([0, deg] + [deg] * deg), np.arange(1, deg + 1))
    x, y = R.walk_draws(9, 3, 6, 2)
    tr = R.walk([csr], [0, 0], [0] * 6, None, 9, 3)
    for i in range(6):
        assert tr[i, 1] == 1 + (int(x[i, 0]) >> 16)           # x, scaled by mulhi
    loop = (np.array([0, deg]), np.zeros(deg, np.int64))        # node 0 -> node 0, deg times
    for thr in (2 ** 31, 2 ** 30):
        tr = R.walk([loop], [0, 0], [0] * 6, [thr, 0], 9, 3)
        for i in range(6):
            assert (tr[i, 2] == -1) == (int(y[i, 0]) < thr)   # y against the threshold
            assert tr[i, 1] == 0


def test_walk_cases():
    indptr = np.array([0, 2, 3, 3, 4])       # 0 -> {1, 2}, 1 -> {3}, 2 -> {}, 3 -> {0}
    indices = np.array([1, 2, 3, 0])
    tr = R.walk([(indptr, indices)], [0] * 4, [2, 1, 9, -1, 3], None, 5)
    assert tr[0].tolist() == [2, -1, -1, -1, -1]       # a dead end at once
    assert tr[1, :3].tolist() == [1, 3, 0] and tr[1, 3] in (1, 2)
    assert tr[2].tolist() == [9, -1, -1, -1, -1] and tr[3].tolist() == [-1, -1, -1, -1, -1]
    assert tr[4, :2].tolist() == [3, 0]
    always = [R.threshold(1.0)] * 4
    tr = R.walk([(indptr, indices)], [0] * 4, [1, 3], always, 5)
    assert tr.tolist() == [[1, 3, -1, -1, -1], [3, 0, -1, -1, -1]]
    step = [0, R.threshold(1.0), 0, 0]                 # stops after step 1: column 2 is the last
    tr = R.walk([(indptr, indices)], [0] * 4, [1, 3], step, 5)
    assert tr[0].tolist() == [1, 3, 0, -1, -1] and tr[1, 3] == -1 and tr[1, 2] in (1, 2)
    assert R.walk([(indptr, indices)], [], [1, 2], None, 5).tolist() == [[1], [2]]


def test_visit_topk_cases():
    tr = np.array([[0, 5, 7], [0, 5, 3], [0, -1, -1], [0, 3, 3],
                   [1, -1, -1], [1, -1, -1], [1, -1, -1], [1, -1, -1]])
    nbr, cnt, num = R.visit_topk(tr, 4, 1, 1, 3)
    assert nbr[0].tolist() == [3, 5, 7] and cnt[0].tolist() == [3, 2, 1] and num[0] == 3
    assert nbr[1].tolist() == [-1] * 3 and cnt[1].tolist() == [0] * 3 and num[1] == 0
    nbr, cnt, num = R.visit_topk(tr, 4, 2, 1, 2)
    assert nbr[0].tolist() == [3, 7] and cnt[0].tolist() == [2, 1]      # column 2 only
    nbr, cnt, num = R.visit_topk(tr, 4, 0, 2, 4)
    assert nbr[0].tolist() == [0, 3, 7, -1] and cnt[0].tolist() == [4, 2, 1, 0]  # ties by id


def _stat(counts, expect):
    return float(((counts - expect) ** 2 / expect).sum())


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("deg,walks,bins", [(12, 20000, 12), (5000, 20000, 50)])
def test_first_step_is_uniform(deg, walks, bins, seed):
    x, _ = R.walk_draws(seed, 0, walks, 1)
    pos = (x[:, 0].astype(object) * deg) >> 32
    c = np.bincount(np.asarray(pos, np.int64) // (deg // bins), minlength=bins)
    assert c.sum() == walks and len(c) == bins
    stat, bound = _stat(c, walks / bins), _chi2_quantile(bins - 1)
    print("chi2 first step deg=%d seed=%d: %.2f (bound %.2f)" % (deg, seed, stat, bound))
    assert stat < bound


@pytest.mark.parametrize("seed", SEEDS)
def test_trace_lengths_are_geometric(seed):
    """On a self-loop no walk meets a dead end, so with p = 0.3 at every step a walk of at
    most L steps makes n steps with probability q^(n - 1) p for n < L and q^(L - 1) for L."""
    p, L, walks = 0.3, 12, 20000
    loop = (np.array([0, 1]), np.array([0]))
    tr = R.walk([loop], [0] * L, [0] * walks, [R.threshold(p)] * L, seed)
    steps = (tr >= 0).sum(1) - 1
    assert steps.min() >= 1
    pq = R.threshold(p) / 2.0 ** 32
    prob = np.array([(1 - pq) ** (n - 1) * pq for n in range(1, L)] + [(1 - pq) ** (L - 1)])
    c = np.bincount(steps, minlength=L + 1)[1:]
    stat, bound = _stat(c, walks * prob), _chi2_quantile(L - 1)
    print("chi2 trace lengths seed=%d: %.2f (bound %.2f)" % (seed, stat, bound))
    assert stat < bound
