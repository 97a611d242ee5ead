"""Neighbour sampling without a GPU: the names, every host-side validation error of
``dgl.sampling.sample_neighbors`` / ``to_block`` / ``in_subgraph`` (raised before any launch,
so host graphs and host ids reach them), and the uniformity of the contract's algorithm,
checked on the numpy restatement (``sampling_ref.py``) alone.

Uniformity.  Pearson's statistic of the neighbour counts is compared with the 1 - 1e-6
quantile of chi-square with (bins - 1) degrees of freedom, computed here.  Without
replacement the counts of one seed are negatively correlated (they sum to the fan-out), which
makes the statistic's expectation smaller than chi-square's, not larger: sum_j (O_j - n q)^2
/ (n q) has expectation (bins)(1 - q) at inclusion rate q, so the bound stays valid.  The RNG
seeds are named below (SEEDS); the restatement passes with each of them."""
import os
import sys

import numpy as np
import pytest
import torch as th

import dgl
from dgl import kernel as K

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_ref as R  # noqa: E402

SEEDS = (20261021, 7, 0x5EED5EED5EED)


def test_names_are_importable():
    from dgl.sampling import sample_neighbors
    from dgl.transform import to_block, in_subgraph, out_subgraph
    assert dgl.sampling.sample_neighbors is sample_neighbors
    assert dgl.to_block is to_block and dgl.in_subgraph is in_subgraph
    assert dgl.out_subgraph is out_subgraph
    assert dgl.NID == dgl.EID == "_ID"
    for name in ("sample_neighbors", "csr_gather_rows", "block_relabel", "sample_max_fanout"):
        assert callable(getattr(K, name))
    assert K.sample_max_fanout() >= 64


def _g():
    g = dgl.DGLGraph()
    g.add_nodes(6)
    g.add_edges([0, 1, 2, 3, 4], [1, 2, 3, 4, 5])
    return g


@pytest.fixture
def no_launch(monkeypatch):
    """Fail the test if anything reaches the library's launching entries."""
    def boom(*a, **k):
        raise AssertionError("a launch was attempted before validation finished")
    for name in ("sample_neighbors", "csr_gather_rows", "block_relabel"):
        monkeypatch.setattr(K, name, boom)


def test_prob_is_not_built(no_launch):
    with pytest.raises(dgl.DGLError, match="weighted sampling"):
        dgl.sampling.sample_neighbors(_g(), [1], 2, prob="p")


def test_fanout_above_limit_names_the_limit(no_launch):
    with pytest.raises(dgl.DGLError, match="limit of %d" % K.sample_max_fanout()):
        dgl.sampling.sample_neighbors(_g(), [1], K.sample_max_fanout() + 1)


@pytest.mark.parametrize("fanout", [-1, -5])
def test_negative_fanout(no_launch, fanout):
    with pytest.raises(dgl.DGLError, match="must not be negative"):
        dgl.sampling.sample_neighbors(_g(), [1], fanout)


@pytest.mark.parametrize("fanout", [2.0, "3", None, True])
def test_fanout_must_be_an_int(no_launch, fanout):
    with pytest.raises(dgl.DGLError, match="fanout must be an int"):
        dgl.sampling.sample_neighbors(_g(), [1], fanout)


@pytest.mark.parametrize("edge_dir", ["both", "IN", None, 0])
def test_bad_edge_dir(no_launch, edge_dir):
    with pytest.raises(dgl.DGLError, match="edge_dir must be 'in' or 'out'"):
        dgl.sampling.sample_neighbors(_g(), [1], 2, edge_dir=edge_dir)


@pytest.mark.parametrize("nodes", [[6], [-1], [0, 1, 99], th.tensor([2, 6]), np.array([-3])])
def test_host_seed_out_of_range(no_launch, nodes):
    with pytest.raises(dgl.DGLError, match="out of range"):
        dgl.sampling.sample_neighbors(_g(), nodes, 2)


def test_host_seed_range_follows_edge_dir(no_launch):
    g = dgl.bipartite(([0, 1, 2], [0, 0, 1]), num_nodes=(5, 2))
    with pytest.raises(dgl.DGLError, match=r"out of range \[0, 2\)"):
        dgl.sampling.sample_neighbors(g, [3], 2, edge_dir="in")
    with pytest.raises(dgl.DGLError, match=r"out of range \[0, 5\)"):
        dgl.sampling.sample_neighbors(g, [5], 2, edge_dir="out")


def test_float_ids(no_launch):
    with pytest.raises(dgl.DGLError, match="must hold integers"):
        dgl.sampling.sample_neighbors(_g(), th.tensor([1.0]), 2)
    with pytest.raises(dgl.DGLError, match="must hold integers"):
        dgl.in_subgraph(_g(), [0.5])


def test_bad_seed(no_launch):
    with pytest.raises(dgl.DGLError, match="seed must be an int"):
        dgl.sampling.sample_neighbors(_g(), [1], 2, seed=1.5)


def test_multi_relation_input(no_launch):
    g = dgl.heterograph({("a", "x", "b"): ([0], [0]), ("b", "y", "a"): ([0], [0])})
    with pytest.raises(dgl.DGLError, match="more than one edge type"):
        dgl.sampling.sample_neighbors(g, [0], 2)
    with pytest.raises(dgl.DGLError, match="more than one edge type"):
        dgl.to_block(g, [0])
    with pytest.raises(dgl.DGLError, match="more than one edge type"):
        dgl.in_subgraph(g, [0])
    with pytest.raises(dgl.DGLError, match="DGLGraph or a DGLHeteroGraph"):
        dgl.sampling.sample_neighbors("graph", [0], 2)


def test_no_device(no_launch, monkeypatch):
    monkeypatch.setattr(th.cuda, "is_available", lambda: False)
    with pytest.raises(dgl.DGLError, match="ROCm devices only"):
        dgl.sampling.sample_neighbors(_g(), [1], 2)
    with pytest.raises(dgl.DGLError, match="ROCm devices only"):
        dgl.to_block(_g(), [1])
    with pytest.raises(dgl.DGLError, match="ROCm devices only"):
        dgl.out_subgraph(_g(), [1])


def test_to_block_host_ids_out_of_range(no_launch):
    with pytest.raises(dgl.DGLError, match="out of range"):
        dgl.to_block(_g(), [6])
    with pytest.raises(dgl.DGLError, match="out of range"):
        dgl.out_subgraph(_g(), [-1])


# ---- the restatement itself ----------------------------------------------------------
def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    z = R.philox4x32_10(0, 0, 0, 0, 0, 0)
    assert [int(v) for v in z] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = 0xFFFFFFFF
    o = R.philox4x32_10(f, f, f, f, f, f)
    assert [int(v) for v in o] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    p = R.philox4x32_10(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0)
    assert [int(v) for v in p] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_draw_layout():
    """Draw t of slot i: component t & 3 of the block at counter rng_ctr + (t >> 2), slot i."""
    r = R.draws(0x1234567890ABCDEF, 2 ** 32 - 1, [0, 5, 2 ** 33 + 1], 7)
    for row, slot in enumerate([0, 5, 2 ** 33 + 1]):
        for t in range(7):
            c = 2 ** 32 - 1 + (t >> 2)
            blk = R.philox4x32_10(c & 0xFFFFFFFF, c >> 32, slot & 0xFFFFFFFF, slot >> 32,
                                  0x90ABCDEF, 0x12345678)
            assert int(r[row, t]) == int(blk[t & 3])


def test_count_rule_and_cases():
    indptr = [0, 0, 1, 5, 12]
    indices = np.arange(12) * 3
    data = np.arange(12)[::-1]
    seeds = [3, 0, 1, 2, 3, 7]
    off, nbr, eid = R.sample(indptr, indices, data, seeds, 4, False, 1)
    assert off.tolist() == [0, 4, 4, 5, 9, 13, 13]
    assert nbr[4:5].tolist() == [0] and nbr[5:9].tolist() == [3, 6, 9, 12]  # whole rows
    for a, b in zip(off[:-1], off[1:]):
        assert np.all(np.diff(nbr[a:b]) > 0)  # sorted, no repeats
    assert np.array_equal(eid, 11 - nbr // 3)
    off, nbr, _ = R.sample(indptr, indices, data, seeds, 4, True, 1)
    assert off.tolist() == [0, 4, 4, 8, 12, 16, 16]
    assert nbr[4:8].tolist() == [0] * 4
    for a, b in zip(off[:-1], off[1:]):
        assert np.all(np.diff(nbr[a:b]) >= 0)
    assert R.sample(indptr, indices, data, seeds, 0, True, 1)[0].tolist() == [0] * 7


def test_relabel_order():
    src_nodes, new_src, uniq = R.relabel([3, 2], [2, 1])
    assert src_nodes.tolist() == [3, 2, 1] and new_src.tolist() == [1, 2] and uniq == 2
    src_nodes, new_src, uniq = R.relabel([3, 2], [2, 1], include_dst=False)
    assert src_nodes.tolist() == [2, 1] and new_src.tolist() == [0, 1] and uniq == 0
    assert R.relabel([4, 4, 1], [])[2] == 2


def _chi2_quantile(df, tail=1e-6):
    try:
        from scipy import stats
        return float(stats.chi2.isf(tail, df))
    except ImportError:  # Wilson-Hilferty: chi2_df ~ df (1 - 2/(9 df) + z sqrt(2/(9 df)))^3
        z = 4.753424308822899  # the 1 - 1e-6 quantile of the standard normal
        a = 2.0 / (9.0 * df)
        return df * (1.0 - a + z * a ** 0.5) ** 3


def _counts(deg, fanout, replace, slots, seed, bins):
    r = R.draws(seed, 0, np.arange(slots), fanout)
    c = np.zeros(bins, np.int64)
    width = deg // bins
    for i in range(slots):
        picks = R.pick_positions(r[i], deg, fanout, replace)
        assert len(picks) == fanout
        if not replace:
            assert len(set(picks)) == fanout
        np.add.at(c, np.asarray(picks) // width, 1)
    return c


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("replace", [True, False])
@pytest.mark.parametrize("deg,fanout,slots,bins", [(12, 5, 4000, 12), (5000, 10, 4000, 50)])
def test_uniform(deg, fanout, slots, bins, replace, seed):
    c = _counts(deg, fanout, replace, slots, seed, bins)
    assert c.sum() == slots * fanout
    expect = slots * fanout / bins  # without replacement: slots x inclusion rate fanout / deg
    stat = float(((c - expect) ** 2 / expect).sum())
    bound = _chi2_quantile(bins - 1)
    print("chi2 deg=%d fanout=%d replace=%s seed=%d: %.2f (bound %.2f)"
          % (deg, fanout, replace, seed, stat, bound))
    assert stat < bound
