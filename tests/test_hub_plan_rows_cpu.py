"""The hub plan's row starts (build_hub_plan's ``starts`` / ``start_rank`` / ``row_ids``,
DGLMIHubPlan) on CPU tensors, at test_hub_plan_cpu's three shapes: the bitmap's set bits
are exactly the positions where ``rows`` changes, ``start_rank`` is its exclusive prefix
popcount per word, ``row_ids`` the rows in walk order, the padding word zero -- also when
the last word is full (nnz a multiple of 32) and when it holds one bit (nnz = 33)."""
import numpy as np
import pytest
import torch as th

from dgl.graph_index import build_hub_plan, plan_row_starts


def _csr(n, m, seed, skew=1.1):
    rs = np.random.RandomState(seed)
    dst = np.sort((rs.pareto(skew, m) * 3).astype(np.int64) % n)
    src = (rs.pareto(skew, m) * 5).astype(np.int64) % n
    order = np.lexsort((src, dst))
    dst, src = dst[order], src[order]
    indptr = np.zeros(n + 1, np.int64)
    indptr[1:] = np.cumsum(np.bincount(dst, minlength=n))
    t = lambda a: th.from_numpy(a.astype(np.int32))
    return t(indptr), t(src), t(dst)


def _check(p, nnz):
    rows = p["rows"].long()
    assert rows.shape[0] == nnz
    words = (nnz + 31) // 32
    starts, rank, ids = p["starts"], p["start_rank"], p["row_ids"]
    assert starts.dtype == th.int32 and rank.dtype == th.int32 and ids.dtype == th.int32
    assert starts.shape[0] == words + 1 and rank.shape[0] == words + 1
    # bit p & 31 of word p >> 5, every position and the padding word's 32
    w = starts.long() & 0xFFFFFFFF
    flags = ((w[:, None] >> th.arange(32)[None, :]) & 1).reshape(-1)
    want = th.ones(nnz, dtype=th.int64)
    want[1:] = (rows[1:] != rows[:-1]).long()
    assert th.equal(flags[:nnz], want)
    assert int(flags[nnz:].sum()) == 0 and int(starts[-1]) == 0
    per_word = flags.reshape(-1, 32).sum(1)
    assert th.equal(rank.long(), th.cumsum(per_word, 0) - per_word)
    assert th.equal(ids.long(), th.unique_consecutive(rows))
    assert ids.shape[0] == int(want.sum())


@pytest.mark.parametrize("n,m,deg,nb", [(500, 20_000, 16, 8), (64, 3_000, 1, 8), (300, 5_000, 40, 4)])
def test_row_starts_of_a_plan(n, m, deg, nb):
    indptr, cols, rows = _csr(n, m, seed=n)
    _check(build_hub_plan(indptr, cols, rows, deg, nb), m)


@pytest.mark.parametrize("m", [32, 33, 64, 4_096, 4_097])
def test_last_word_full_and_one_bit(m):
    """nnz a multiple of 32: the last word is full and the padding word follows it;
    nnz = 33: the last word holds one position."""
    indptr, cols, rows = _csr(16, m, seed=m)
    _check(build_hub_plan(indptr, cols, rows, 2, 8), m)


def test_starts_of_given_rows():
    """Bit 31 of a word (the int32's sign), a start at every position, none but the first."""
    rows = th.cat([th.zeros(31), th.arange(1, 34), th.full((64,), 40)]).to(th.int32)
    s = plan_row_starts(rows)
    _check(dict(s, rows=rows), 128)
    assert s["starts"].tolist() == [-2 ** 31 | 1, -1, 1, 0, 0]
    assert s["start_rank"].tolist() == [0, 2, 34, 35, 35]
    one = plan_row_starts(th.full((70,), 7, dtype=th.int32))
    assert one["starts"].tolist() == [1, 0, 0, 0] and one["row_ids"].tolist() == [7]
