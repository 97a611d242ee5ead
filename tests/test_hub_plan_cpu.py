"""build_hub_plan on CPU tensors: the plan's positions are a permutation of the CSR's,
ordered (source block, row, original position) in the hub part and unchanged in the light
part; indptr agrees with rows; the quantile blocks hold equal shares of the hub edges up
to one source's count."""
import numpy as np
import pytest
import torch as th

from dgl.graph_index import build_hub_plan


def _csr(n, m, seed, skew=1.1):
    rs = np.random.RandomState(seed)
    dst = np.sort((rs.pareto(skew, m) * 3).astype(np.int64) % n)
    src = (rs.pareto(skew, m) * 5).astype(np.int64) % n
    # rows list their sources ascending, as the in-CSR does
    order = np.lexsort((src, dst))
    dst, src = dst[order], src[order]
    indptr = np.zeros(n + 1, np.int64)
    indptr[1:] = np.cumsum(np.bincount(dst, minlength=n))
    t = lambda a: th.from_numpy(a.astype(np.int32))
    return t(indptr), t(src), t(dst)


@pytest.mark.parametrize("n,m,deg,nb", [(500, 20_000, 16, 8), (64, 3_000, 1, 8), (300, 5_000, 40, 4)])
def test_plan_order(n, m, deg, nb):
    indptr, cols, rows = _csr(n, m, seed=n)
    p = build_hub_plan(indptr, cols, rows, deg, nb)
    pos, prow, nh, h = p["positions"], p["rows"].long(), p["num_hubs"], p["hub_nnz"]
    virt = nb * nh
    assert th.equal(th.sort(pos).values, th.arange(m))
    assert th.equal(p["indices"], cols[pos])
    degs = (indptr[1:] - indptr[:-1]).long()
    assert th.equal(p["hub_rows"].long(), th.nonzero(degs >= deg).reshape(-1))
    assert h == int(degs[degs >= deg].sum()) and 0 < h
    # hub part: virtual rows, ascending = block-major then row-major, original order within
    assert bool((prow[:h] < virt).all()) and bool((prow[h:] >= virt).all())
    assert th.equal(p["hub_rows"].long()[prow[:h] % nh], rows[pos[:h]].long())
    key = prow[:h] * m + pos[:h]
    assert bool((key[1:] > key[:-1]).all())
    # a block is a contiguous column range
    block = prow[:h] // nh
    c = cols[pos[:h]].long()
    for b in range(nb - 1):
        if bool((block == b).any()) and bool((block > b).any()):
            assert int(c[block == b].max()) < int(c[block > b].min())
    # light part: the CSR's order, rows shifted
    assert bool((pos[h:][1:] > pos[h:][:-1]).all())
    assert th.equal(prow[h:] - virt, rows[pos[h:]].long())
    # indptr
    ptr = p["indptr"].long()
    assert ptr.shape[0] == virt + n + 1 and int(ptr[0]) == 0 and int(ptr[-1]) == m
    assert th.equal(ptr[1:] - ptr[:-1], th.bincount(prow, minlength=virt + n))
    assert th.equal(ptr[virt + p["hub_rows"].long() + 1] - ptr[virt + p["hub_rows"].long()],
                    th.zeros(nh, dtype=th.int64))
    # quantile blocks: block b starts within one source's count of b * h / nb
    count = th.bincount(c, minlength=n)
    starts = ptr[0:virt + 1:nh]
    for b in range(1, nb):
        first = c[block >= b]
        if first.numel():
            assert 0 <= b * h // nb - int(starts[b]) < int(count[first.min()])


def test_no_hub():
    indptr, cols, rows = _csr(200, 1_000, seed=1)
    assert build_hub_plan(indptr, cols, rows, 10_000, 8) is None
