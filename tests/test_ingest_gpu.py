"""The device graph ingest (csrc/ingest.hip) against tests/ingest_ref.py, array for array.

Every block, relation, typed graph and partition is built by ``device_block_gidx``: two
COO -> CSR sorts and two row expansions, 32- or 64-bit.  The kernels' own tests take their
reference from those CSRs, so a wrong CSR passes them.  Here ``indptr``, ``indices``,
``data`` and ``rows`` of the 32-bit and the 64-bit entries are compared with the numpy
restatement (itself checked against the host ingest in tests/test_ingest_ref_cpu.py) for
equality, dtypes included, on

* row counts on and next to powers of two, with edges in the top rows (the radix sort's
  key width), no edges, one edge, one populated row, 2^20 rows of 5 edges, 100 000 empty
  rows in a run, heavy parallel edges (stability), rectangular blocks, an explicit
  ``data`` argument;
* one item count past the cap of the kernels' grids (the grid-stride loops' second turn);
* the 64-bit entries with the batch length (DGLMI_INGEST_BATCH) at 1 .. nnz + 1: batch
  seams inside rows, on row starts, a last batch of one position, rows filled from many
  batches -- what a graph of 2^31 edges does at 2^30, at a few thousand edges.

No kernel here bound-checks an id: every id of ingest_ref's cases is in range
(test_case_list_holds_what_it_says).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch as th

import ingest_ref as R
from dgl import _ffi
from dgl.graph_index import (device_block_gidx, device_coo_to_csr, device_coo_to_csr64,
                             device_expand_rows)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDE = {32: th.int32, 64: th.int64}
BUILD = {32: device_coo_to_csr, 64: device_coo_to_csr64}


def _dev(a, dtype=th.int32):
    return th.tensor(a).to(DEV, dtype)  # a copy: the shared references are read-only


def _equal(got, want, dtype, what):
    assert got.dtype == dtype, (what, got.dtype)
    assert tuple(got.shape) == want.shape, (what, tuple(got.shape), want.shape)
    g = got.cpu().numpy().astype(np.int64)
    if not np.array_equal(g, want):
        bad = np.flatnonzero(g != want)
        raise AssertionError("%s: %d of %d differ, first at %d: got %d, expected %d"
                             % (what, len(bad), len(want), bad[0], g[bad[0]], want[bad[0]]))


def _check_csr(got, want, bits, what):
    """(indptr, indices, data[, rows]): offsets and edge ids in the entry's width, node
    ids int32."""
    for g, w, part, dt in zip(got, want, ("indptr", "indices", "data", "rows"),
                              (WIDE[bits], th.int32, WIDE[bits], th.int32)):
        _equal(g, w, dt, "%s %s" % (what, part))


def _check_entries(bits, n, row, col, data, what):
    """One COO -> CSR call and its row expansion against the reference."""
    want = R.coo_to_csr(n, row, col, data)
    d = None if data is None else _dev(data, WIDE[bits])
    got = BUILD[bits](n, _dev(row), _dev(col), d)
    _check_csr(got, want, bits, what)
    _equal(device_expand_rows(got[0], len(row)), R.expand_rows(want[0]), th.int32, what + " rows")
    return got


def _check_block(bits, num_src, num_dst, src, dst, want=None, what="block"):
    gidx = device_block_gidx(num_src, num_dst, _dev(src), _dev(dst), bits=bits)
    assert gidx.num_bits == bits
    want = want or R.block(num_src, num_dst, src, dst)
    for c, w, name in ((gidx.in_csr, want[0], "in-CSR"), (gidx.out_csr, want[1], "out-CSR")):
        _check_csr((c.indptr, c.indices, c.data, c.rows), w, bits, "%s %s" % (what, name))
    assert (gidx.in_csr.num_rows, gidx.in_csr.num_cols) == (num_dst, num_src)
    assert (gidx.out_csr.num_rows, gidx.out_csr.num_cols) == (num_src, num_dst)
    return gidx


@pytest.mark.parametrize("name", list(R.CASES))
@pytest.mark.parametrize("bits", [32, 64])
def test_entries_match_reference(name, bits, monkeypatch):
    """device_coo_to_csr / device_coo_to_csr64 and device_expand_rows, sorting by either
    end, with the edge ids and with an explicit ``data``."""
    monkeypatch.delenv("DGLMI_INGEST_BATCH", raising=False)
    num_src, num_dst, src, dst = R.case(name)
    for n, row, col, side in ((num_src, src, dst, "by src"), (num_dst, dst, src, "by dst")):
        for data in (None, R.edge_data(len(src))):
            got = _check_entries(bits, n, row, col, data,
                                 "%s %s%s" % (name, side, "" if data is None else " data"))
            if len(src) == 0:
                assert got[0].shape == (n + 1,) and not got[0].any()


@pytest.mark.parametrize("name", list(R.CASES))
@pytest.mark.parametrize("bits", [32, 64])
def test_block_matches_reference(name, bits, monkeypatch):
    monkeypatch.delenv("DGLMI_INGEST_BATCH", raising=False)
    _check_block(bits, *R.case(name), what=name)


@pytest.mark.parametrize("bits", [32, 64])
def test_parallel_edges_keep_edge_id_order(bits, monkeypatch):
    """Within equal (row, col) the returned edge ids ascend -- stated on the device arrays
    themselves, for the sort by either end and for both CSRs of the block."""
    monkeypatch.delenv("DGLMI_INGEST_BATCH", raising=False)
    num_src, num_dst, src, dst = R.case("parallel_edges")

    def ascending(indptr, indices, data, ncols):
        rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr.cpu().numpy()))
        key = rows * ncols + indices.cpu().numpy().astype(np.int64)
        order = np.argsort(key, kind="stable")  # position order kept inside a pair
        k, d = key[order], data.cpu().numpy()[order]
        same = k[1:] == k[:-1]
        assert same.sum() >= 3000 - 40
        assert (d[1:][same] > d[:-1][same]).all()
        assert np.array_equal(np.sort(d), np.arange(len(d)))

    ascending(*BUILD[bits](num_src, _dev(src), _dev(dst)), num_dst)
    ascending(*BUILD[bits](num_dst, _dev(dst), _dev(src)), num_src)
    gidx = device_block_gidx(num_src, num_dst, _dev(src), _dev(dst), bits=bits)
    ascending(gidx.in_csr.indptr, gidx.in_csr.indices, gidx.in_csr.data, num_src)
    ascending(gidx.out_csr.indptr, gidx.out_csr.indices, gidx.out_csr.data, num_dst)


def test_workspace_contract(monkeypatch):
    """At least 256 bytes for an empty graph; one byte less than asked for is refused (before
    any launch: the outputs keep their fill)."""
    monkeypatch.delenv("DGLMI_INGEST_BATCH", raising=False)
    L = _ffi.lib()
    for n in (0, 1, 7):
        assert L.DGLMICOOToCSRDeviceWorkspaceBytes(n, 0) >= 256
        assert L.DGLMICOOToCSRDevice64WorkspaceBytes(n, 0) >= 256
    n, _, src, dst = R.case("bits_n257")
    m = len(src)
    row, col = _dev(src), _dev(dst)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(th.cuda.current_stream(DEV).cuda_stream)
    for bits, size, fn in ((32, L.DGLMICOOToCSRDeviceWorkspaceBytes, L.DGLMICOOToCSRDevice),
                           (64, L.DGLMICOOToCSRDevice64WorkspaceBytes, L.DGLMICOOToCSRDevice64)):
        need = int(size(n, m))
        assert need >= 256
        ws = th.empty(need, dtype=th.uint8, device=DEV)
        indptr = th.full((n + 1,), -7, dtype=WIDE[bits], device=DEV)
        indices = th.full((m,), -7, dtype=th.int32, device=DEV)
        out = th.full((m,), -7, dtype=WIDE[bits], device=DEV)
        rc = fn(n, m, p(row), p(col), None, p(indptr), p(indices), p(out), p(ws), need - 1, stream)
        assert rc != 0
        th.cuda.synchronize()
        assert bool((indptr == -7).all()) and bool((indices == -7).all()) and bool((out == -7).all())
        rc = fn(n, m, p(row), p(col), None, p(indptr), p(indices), p(out), p(ws), need, stream)
        assert rc == 0
        _check_csr((indptr, indices, out), R.coo_to_csr(n, src, dst), bits, "exact workspace")


# ---- past the grid cap ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _grid_tail():
    """The GRID_TAIL_NNZ-edge graph and its reference block, built once and never written."""
    case = R.grid_tail()
    want = R.block(*case)
    for part in case[2:] + want[0] + want[1]:
        part.setflags(write=False)
    return case, want


@pytest.mark.parametrize("bits", [32, 64])
def test_grid_tail(bits, monkeypatch):
    """ingest_ref.GRID_TAIL_NNZ = 16384 * 256 + 3 items, the cap of grid_of times the block
    plus three: k_iota, k_gather_cols, k_indptr_from_sorted (nnz + 1 items), k_count_rows64,
    k_run_starts, k_scatter_batch64 and k_advance_fill loop a second time, the fill of the
    row expansion too.  The 64-bit entry sorts it as one batch (the default length)."""
    monkeypatch.delenv("DGLMI_INGEST_BATCH", raising=False)
    (num_src, num_dst, src, dst), want = _grid_tail()
    assert len(src) == 16384 * 256 + 3
    got = BUILD[bits](num_src, _dev(src), _dev(dst))
    _check_csr(got, want[1][:3], bits, "grid tail")
    _equal(device_expand_rows(got[0], len(src)), want[1][3], th.int32, "grid tail rows")
    del got
    _check_block(bits, num_src, num_dst, src, dst, want, "grid tail")


def test_grid_tail_in_batches_of_2p20(monkeypatch):
    """The same graph through the 64-bit entries in four full batches of 2^20 positions
    and a last one of three: the seam logic at a size where every batch fills many blocks."""
    monkeypatch.setenv("DGLMI_INGEST_BATCH", str(1 << 20))
    (num_src, num_dst, src, dst), want = _grid_tail()
    assert len(src) == 4 * (1 << 20) + 3
    _check_block(64, num_src, num_dst, src, dst, want, "grid tail, B = 2^20")


# ---- batch seams (64-bit entries) ---------------------------------------------------------

def _seam_batches(nnz):
    return [2, 7, 64, 1000, nnz - 1, nnz, nnz + 1]


@pytest.mark.parametrize("name,batches", [("seam_300", [1] + _seam_batches(300)),
                                          ("seam_6000", _seam_batches(6000))])
def test_batch_seams_coo_to_csr64(name, batches, monkeypatch):
    """DGLMICOOToCSRDevice64 / DGLMICSRExpandRows64 with the batch length from 1 (the
    300-edge graph only: four launches, a sort and a scan per batch) to nnz + 1: the
    arrays equal the reference at every length, hence each other.  Rows of the graph
    interleave over the edge list, so the long rows get a run from every batch (the
    per-row cursor of k_scatter_batch64 / k_advance_fill)."""
    num_src, num_dst, src, dst = R.case(name)
    nnz = len(src)
    assert batches[-3:] == [nnz - 1, nnz, nnz + 1]
    data = R.edge_data(nnz)
    first = None
    for b in batches:
        monkeypatch.setenv("DGLMI_INGEST_BATCH", str(b))
        got = []
        for n, row, col in ((num_src, src, dst), (num_dst, dst, src)):
            for d in (None, data):
                g = _check_entries(64, n, row, col, d, "%s B=%d" % (name, b))
                got.extend(g)
        if first is None:
            first = got
        for a, c in zip(first, got):
            assert th.equal(a, c), "B=%d differs from B=%d" % (b, batches[0])


@pytest.mark.parametrize("name,batches", [("seam_300", [1] + _seam_batches(300)),
                                          ("seam_6000", _seam_batches(6000))])
def test_batch_seams_block64(name, batches, monkeypatch):
    """device_block_gidx(bits=64) at every batch length: the second sort takes the first
    one's edge ids as ``data`` and its expanded rows as columns."""
    case = R.case(name)
    want = R.block(*case)
    for b in batches:
        monkeypatch.setenv("DGLMI_INGEST_BATCH", str(b))
        _check_block(64, *case, want=want, what="%s B=%d" % (name, b))


# rows 1, 4, 5, 7 and 8 of 9 hold positions [0,5) [5,12) [12,13) [13,20) [20,21)
SEAM_INDPTR = np.array([0, 0, 5, 5, 5, 12, 13, 13, 20, 21], np.int64)


def _seams(b, nnz=21):
    return list(range(b, nnz, b))


def test_expand_rows64_seam_batches_are_what_they_claim():
    starts = set(SEAM_INDPTR[:-1][np.diff(SEAM_INDPTR) > 0].tolist()) - {0}
    assert starts == {5, 12, 13, 20}
    assert 3 in _seams(3) and 3 not in starts                  # inside a row
    assert 5 in _seams(5) and 5 in starts                      # on a row's first position
    assert 6 in _seams(6) and 5 in starts                      # just after one
    assert _seams(5)[-1] == 20 and _seams(4)[-1] == 20         # a last batch of one position
    assert _seams(21) == [] and _seams(22) == []


@pytest.mark.parametrize("b", [1, 2, 3, 4, 5, 6, 7, 10, 13, 20, 21, 22])
def test_expand_rows64_across_seams(b, monkeypatch):
    """DGLMICSRExpandRows64 on a hand-built indptr: B = 3 cuts row 1 in the middle, B = 5
    puts seams on the first positions of rows 4 and 8, B = 6 one position after row 4's
    start and on row 5's only position, B = 4, 5, 10 and 20 leave a last batch of one
    position, B = 13 starts its second batch on the row after a one-position row, B = 1
    makes every position a batch; 21 and 22 are a single batch."""
    monkeypatch.setenv("DGLMI_INGEST_BATCH", str(b))
    want = R.expand_rows(SEAM_INDPTR)
    assert np.array_equal(want, np.repeat(np.arange(9), np.diff(SEAM_INDPTR)))
    rows = device_expand_rows(_dev(SEAM_INDPTR, th.int64), 21)
    _equal(rows, want, th.int32, "B=%d" % b)
    # the 32-bit entry has no batches: the knob must not reach it
    _equal(device_expand_rows(_dev(SEAM_INDPTR, th.int32), 21), want, th.int32, "int32")
