"""The checks of DGLGraph.subgraph / edge_subgraph that need no device."""
import numpy as np
import pytest
import torch as th

import dgl
from dgl._ffi import DGLError


def _cycle():
    g = dgl.DGLGraph()
    g.add_nodes(5)
    g.add_edges([0, 1, 2, 3, 4], [1, 2, 3, 4, 0])
    return g


@pytest.mark.parametrize("nodes, message", [
    ([[0, 1], [2, 3]], "1-D"),
    (np.zeros((2, 2), np.int64), "1-D"),
    (th.zeros(2, 2, dtype=th.int64), "1-D"),
    ([0.0, 1.0], "integers"),
    (th.tensor([0.5, 1.0]), "integers"),
    ([0, 5], "out of range"),
    (th.tensor([-1, 2]), "out of range"),
])
def test_bad_ids_raise_before_any_device_work(nodes, message):
    with pytest.raises(DGLError, match=message):
        _cycle().subgraph(nodes)
    if message != "out of range":  # edge ids are range-checked on the device
        with pytest.raises(DGLError, match=message):
            _cycle().edge_subgraph(nodes)


@pytest.mark.parametrize("call", ["parent_nid", "parent_eid", "copy_from_parent", "copy_to_parent",
                                  "map_to_subgraph_nid"])
def test_bookkeeping_is_for_subgraphs_only(call):
    g = _cycle()
    assert g.parent is None and not hasattr(g, "parent_nid") and not hasattr(g, "parent_eid")
    with pytest.raises(DGLError, match="only support %s for subgraphs" % call):
        attr = getattr(g, call)
        attr() if call.startswith("copy") else attr([0]) if call.startswith("map") else None
