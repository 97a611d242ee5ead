"""dgl.batch / dgl.unbatch and the batch fields of DGLGraph (no GPU: CPU tensors in the
frames; graph.py:4029-4288 of the reference)."""
import warnings

import numpy as np
import pytest
import torch as th

import dgl


def _graph(n, src, dst, seed):
    g = dgl.DGLGraph()
    g.add_nodes(n)
    if len(src):
        g.add_edges(src, dst)
    gen = th.Generator().manual_seed(seed)
    g.ndata["h"] = th.randn(n, 3, generator=gen)
    g.edata["w"] = th.randn(len(src), 2, generator=gen)
    return g


def _three():
    return [_graph(3, [0, 1, 2], [1, 2, 0], 1), _graph(2, [0], [1], 2),
            _graph(4, [0, 0, 3, 2, 1], [1, 2, 0, 3, 3], 3)]


def _edges(g):
    s, d = g.edges()
    return s.tolist(), d.tolist()


def test_batch_counts_edges_and_frames():
    gs = _three()
    bg = dgl.batch(gs)
    assert bg.batch_size == 3
    assert bg.batch_num_nodes == [3, 2, 4]
    assert bg.batch_num_edges == [3, 1, 5]
    assert bg.number_of_nodes() == 9 and bg.number_of_edges() == 9
    src, dst, off = [], [], 0
    for g in gs:
        s, d = _edges(g)
        src += [x + off for x in s]
        dst += [x + off for x in d]
        off += g.number_of_nodes()
    assert _edges(bg) == (src, dst)
    assert bg.edges(form="eid").tolist() == list(range(9))
    assert th.equal(bg.ndata["h"], th.cat([g.ndata["h"] for g in gs]))
    assert th.equal(bg.edata["w"], th.cat([g.edata["w"] for g in gs]))
    # the batch owns its columns: writing to it leaves the inputs alone
    before = gs[0].ndata["h"].clone()
    bg.ndata["h"] = bg.ndata["h"] * 2
    assert th.equal(gs[0].ndata["h"], before)


def test_unbatch_round_trip():
    gs = _three()
    out = dgl.unbatch(dgl.batch(gs))
    assert len(out) == 3
    for a, b in zip(gs, out):
        assert b.batch_size == 1
        assert a.number_of_nodes() == b.number_of_nodes()
        assert _edges(a) == _edges(b)
        assert th.equal(a.ndata["h"], b.ndata["h"])
        assert th.equal(a.edata["w"], b.edata["w"])


def test_unbatched_graph_is_a_batch_of_one():
    g = _three()[2]
    assert g.batch_size == 1
    assert g.batch_num_nodes == [4] and g.batch_num_edges == [5]
    assert dgl.unbatch(g) == [g]


def test_batching_batches_flattens():
    gs = _three() + [_graph(1, [], [], 4)]
    b1, b2 = dgl.batch(gs[:2]), dgl.batch(gs[2:])
    bg = dgl.batch([b1, b2])
    assert bg.batch_size == 4
    assert bg.batch_num_nodes == [3, 2, 4, 1]
    assert bg.batch_num_edges == [3, 1, 5, 0]
    flat = dgl.batch(gs)
    assert _edges(bg) == _edges(flat)
    assert th.equal(bg.ndata["h"], flat.ndata["h"])
    for a, b in zip(gs, dgl.unbatch(bg)):
        assert _edges(a) == _edges(b) and th.equal(a.ndata["h"], b.ndata["h"])


def test_graphs_without_nodes_or_edges():
    gs = [_graph(0, [], [], 1), _graph(3, [], [], 2), _graph(2, [1, 0], [0, 1], 3),
          _graph(0, [], [], 4)]
    bg = dgl.batch(gs)
    assert bg.batch_size == 4
    assert bg.batch_num_nodes == [0, 3, 2, 0]
    assert bg.batch_num_edges == [0, 0, 2, 0]
    assert _edges(bg) == ([4, 3], [3, 4])
    assert th.equal(bg.ndata["h"], th.cat([gs[1].ndata["h"], gs[2].ndata["h"]]))
    assert th.equal(bg.edata["w"], gs[2].edata["w"])
    out = dgl.unbatch(bg)
    assert [g.number_of_nodes() for g in out] == [0, 3, 2, 0]
    assert [g.number_of_edges() for g in out] == [0, 0, 2, 0]
    assert _edges(out[2]) == ([1, 0], [0, 1])
    assert out[0].ndata["h"].shape == (0, 3)


def test_mismatched_attributes_raise():
    gs = _three()
    gs[1].ndata["extra"] = th.zeros(2, 1)
    with pytest.raises(ValueError, match="Expect graph 0 and 1 to have the same node attributes "
                                         "when node_attrs=ALL"):
        dgl.batch(gs)
    bg = dgl.batch(gs, node_attrs="h", edge_attrs=None)
    assert set(bg.ndata.keys()) == {"h"} and len(bg.edata) == 0
    bg = dgl.batch(gs, node_attrs=["h"], edge_attrs=["w"])
    assert set(bg.ndata.keys()) == {"h"} and set(bg.edata.keys()) == {"w"}
    with pytest.raises(ValueError, match="Expected node attrs to be of type None str or Iterable"):
        dgl.batch(gs, node_attrs=3)


def test_local_var_scope_and_to_keep_the_batch():
    bg = dgl.batch(_three())
    lv = bg.local_var()
    assert lv.batch_size == 3 and lv.batch_num_nodes == [3, 2, 4] and lv.batch_num_edges == [3, 1, 5]
    with bg.local_scope():
        bg.ndata["t"] = th.zeros(9, 1)
        assert bg.batch_size == 3
    assert "t" not in bg.ndata and bg.batch_size == 3
    moved = bg.to("cpu")
    assert moved.batch_size == 3 and moved.batch_num_edges == [3, 1, 5]


def test_mutation_resets_the_batch():
    bg = dgl.batch(_three())
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        bg.add_nodes(2)
    assert any("batch_size > 1" in str(w.message) for w in rec)
    assert bg.batch_size == 1
    assert bg.batch_num_nodes == [11] and bg.batch_num_edges == [9]
    bg = dgl.batch(_three())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        bg.add_edges([0], [8])
    assert bg.batch_size == 1 and bg.batch_num_edges == [10]


def test_segment_offsets_cached_per_device():
    bg = dgl.batch(_three())
    off = bg._segments("nodes", "cpu")
    assert off.dtype == th.int64 and off.tolist() == [0, 3, 5, 9]
    assert bg._segments("nodes", "cpu") is off
    assert bg._segments("edges", "cpu").tolist() == [0, 3, 4, 9]
    assert bg.local_var()._segments("nodes", "cpu") is off
    g = _three()[0]
    assert g._segments("nodes", "cpu").tolist() == [0, 3]
    assert np.array_equal(g._segments("edges", "cpu").numpy(), [0, 3])


def test_pickle_leaves_the_segment_cache_behind():
    import pickle
    bg = dgl.batch(_three())
    bg._segments("nodes", "cpu")
    back = pickle.loads(pickle.dumps(bg))
    assert back.__dict__["_segment_cache"] == {} and bg.__dict__["_segment_cache"]
    assert back.batch_num_nodes == [3, 2, 4] and _edges(back) == _edges(bg)
    assert back._segments("nodes", "cpu").tolist() == [0, 3, 5, 9]
