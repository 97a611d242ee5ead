"""The visit-count kernel on the GPU, bit for bit against ``randomwalk_ref.visit_topk``, a
numpy restatement of include/dglmi.h (DGLMIVisitTopK).

Widths are 1, 2 and each side of every padded width ``dgl.kernel.visit_tile`` reports, up
to the maximum; seed counts sit around the instance's seed slots per workgroup.  Rows are
random with repeats, all -1, all one id, all distinct, and engineered count ties; every call
runs twice and the two results are compared bitwise."""
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


def _widths():
    ws, w = {1, 2}, 1
    top = K.visit_max_width()
    while w <= top:
        p = K.visit_tile(w, 1)[0]
        ws.update(x for x in (p - 1, p, p + 1) if 1 <= x <= top)
        w = p + 1
    return sorted(ws)


def _check(traces, wps, col0, col_step, k):
    t = th.from_numpy(np.ascontiguousarray(traces, dtype=np.int64)).to(DEV)
    got = K.visit_topk(t, wps, col0, col_step, k)
    again = K.visit_topk(t, wps, col0, col_step, k)
    assert all(th.equal(a, b) for a, b in zip(got, again))
    assert all(a.dtype == th.int32 for a in got)
    want = R.visit_topk(traces, wps, col0, col_step, k)
    for name, a, b in zip(("nbr", "cnt", "num"), got, want):
        assert np.array_equal(a.cpu().numpy(), b), (name, traces.shape, wps, col0, col_step, k)
    return want


def _rows(rng, seeds, W, kind):
    """(seeds * W, 1) candidates, one column, W walks per seed."""
    n = seeds * W
    if kind == "random":      # repeats with skewed counts, some padding
        x = (rng.pareto(1.0, n) * 3).astype(np.int64) % 50
        x[rng.random(n) < 0.2] = -1
    elif kind == "padding":
        x = np.full(n, -1, np.int64)
    elif kind == "one":
        x = np.full(n, 7, np.int64)
    elif kind == "distinct":
        x = np.concatenate([rng.permutation(W) + 1000 * s for s in range(seeds)]).astype(np.int64)
    else:                      # ties: every id of a seed occurs equally often (or once more)
        x = np.concatenate([rng.permutation(np.arange(W) % 9 + 100) for _ in range(seeds)])
        x = x.astype(np.int64)
    return x.reshape(n, 1)


def test_the_widths_cover_every_instance():
    ws = _widths()
    pads = sorted({K.visit_tile(w, 1)[0] for w in ws})
    assert ws[:2] == [1, 2] and ws[-1] == K.visit_max_width()
    assert pads[-1] >= K.visit_max_width() and len(pads) >= 2
    for p in pads[:-1]:
        assert K.visit_tile(p, 1)[0] == p and K.visit_tile(p + 1, 1)[0] > p


@pytest.mark.parametrize("kind", ["random", "padding", "one", "distinct", "ties"])
def test_every_width(kind):
    rng = np.random.default_rng(5)
    for W in _widths():
        per_wg = K.visit_tile(W, 1)[1]
        for k in (1, 10, K.visit_max_k()):
            _check(_rows(rng, per_wg + 1, W, kind), W, 0, 1, k)


def test_seed_counts_around_a_workgroup():
    rng = np.random.default_rng(6)
    for W in (3, 100, 300, 600, 1500):
        per_wg = K.visit_tile(W, 4)[1]
        for seeds in sorted({1, per_wg - 1, per_wg, per_wg + 1, 2 * per_wg + 1} - {0}):
            _check(_rows(rng, seeds, W, "random"), W, 0, 1, 4)
    t = th.empty((0, 3), dtype=th.int64, device=DEV)
    nbr, cnt, num = K.visit_topk(t, 5, 1, 1, 4)
    assert tuple(nbr.shape) == (0, 4) and tuple(cnt.shape) == (0, 4) and num.numel() == 0


def test_ties_go_to_the_lower_id():
    rows = np.array([[9], [4], [9], [4], [6], [2], [8], [8]])
    nbr, cnt, num = _check(rows, 8, 0, 1, 5)
    assert nbr[0].tolist() == [4, 8, 9, 2, 6] and cnt[0].tolist() == [2, 2, 2, 1, 1]
    nbr, cnt, num = _check(rows, 8, 0, 1, 2)
    assert nbr[0].tolist() == [4, 8] and num[0] == 2
    nbr, cnt, num = _check(rows, 8, 0, 1, 64)
    assert num[0] == 5 and nbr[0, 5:].tolist() == [-1] * 59 and cnt[0, 5:].tolist() == [0] * 59
    big = np.array([[2 ** 31 - 2], [2 ** 31 - 1], [2 ** 40], [0], [-5], [2 ** 31 - 2]])
    nbr, cnt, num = _check(big, 6, 0, 1, 3)          # ids outside [0, 2^31 - 1) are ignored
    assert nbr[0].tolist() == [2 ** 31 - 2, 0, -1] and cnt[0].tolist() == [2, 1, 0]


def test_columns():
    rng = np.random.default_rng(7)
    tr = rng.integers(-1, 12, (6 * 40, 7))
    for col0, step in ((0, 1), (1, 1), (2, 2), (3, 3), (6, 1), (2, 5), (0, 7), (1, 100)):
        _check(tr, 40, col0, step, 6)
    # the PinSAGE shape: every second column from the second on
    want = _check(tr, 40, 2, 2, 6)
    cand = tr[:40, 2::2]
    ids, counts = np.unique(cand[cand >= 0], return_counts=True)
    assert want[1][0, 0] == counts.max()


def test_limits():
    t = th.zeros((8, 4), dtype=th.int64, device=DEV)
    with pytest.raises(dgl.DGLError, match="K must be between 1 and %d" % K.visit_max_k()):
        K.visit_topk(t, 2, 0, 1, K.visit_max_k() + 1)
    with pytest.raises(dgl.DGLError, match="K must be between 1 and"):
        K.visit_topk(t, 2, 0, 1, 0)
    with pytest.raises(dgl.DGLError, match="between 1 and %d candidates" % K.visit_max_width()):
        K.visit_topk(t, 2, 4, 1, 3)                      # no column left
    with pytest.raises(dgl.DGLError, match="col_step must be at least 1"):
        K.visit_topk(t, 2, 0, 0, 3)
    with pytest.raises(dgl.DGLError, match="not a multiple"):
        K.visit_topk(t, 3, 0, 1, 3)
    wide = th.zeros((K.visit_max_width() // 2 + 1, 2), dtype=th.int64, device=DEV)
    with pytest.raises(dgl.DGLError, match="between 1 and %d candidates" % K.visit_max_width()):
        K.visit_topk(wide, wide.shape[0], 0, 1, 3)
