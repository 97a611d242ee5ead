"""tests/ingest_ref.py against the host COOToCSR / CSRTranspose (csrc/ingest.hip, pinned to
the original project's answers in tests/test_host_cpu.py), on the case list that
tests/test_ingest_gpu.py runs through the device ingest: the numpy restatement is checked
here, without a GPU, before any device array is compared with it.  Every comparison is
array equality.

Also the parts of the 64-bit ingest that need no device: the DGLMI_INGEST_BATCH knob's
parsing and the workspace sizes with the knob unset.
"""
import numpy as np
import pytest
import torch as th

import ingest_ref as R
from dgl import _ffi
from dgl.graph_index import host_coo_to_csr, host_csr_transpose


def _same(got, want, what):
    assert len(got) == len(want)
    for g, w, part in zip(got, want, ("indptr", "indices", "data", "rows")):
        assert g.dtype == np.int64 and g.shape == w.shape, (what, part)
        np.testing.assert_array_equal(g, w, err_msg="%s %s" % (what, part))


def _check_case(num_src, num_dst, src, dst):
    m = len(src)
    for n, row, col in ((num_src, src, dst), (num_dst, dst, src)):
        for data in (None, R.edge_data(m)):
            ref = R.coo_to_csr(n, row, col, data)
            _same(ref, host_coo_to_csr(n, row, col, data), "coo_to_csr")
            assert ref[0].shape == (n + 1,) and ref[0][0] == 0 and ref[0][-1] == m
            np.testing.assert_array_equal(R.expand_rows(ref[0]), np.repeat(np.arange(n), np.diff(ref[0])))
    ic, oc = R.block(num_src, num_dst, src, dst)
    h_out = host_coo_to_csr(num_src, src, dst)
    _same(oc[:3], h_out, "out-CSR")
    _same(ic[:3], host_csr_transpose(num_src, num_dst, *h_out), "in-CSR")
    # the in-CSR in words: edges by (destination, source, edge id)
    np.testing.assert_array_equal(ic[2], np.lexsort((np.arange(m), src, dst)))
    np.testing.assert_array_equal(ic[3], dst[ic[2]])
    np.testing.assert_array_equal(oc[3], src[oc[2]])


@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_matches_host_ingest(name):
    _check_case(*R.case(name))


def test_reference_matches_host_ingest_past_the_grid_cap():
    num_src, num_dst, src, dst = R.grid_tail()
    assert len(src) == 16384 * 256 + 3
    ic, oc = R.block(num_src, num_dst, src, dst)
    h_out = host_coo_to_csr(num_src, src, dst)
    _same(oc[:3], h_out, "out-CSR")
    _same(ic[:3], host_csr_transpose(num_src, num_dst, *h_out), "in-CSR")


def test_case_list_holds_what_it_says():
    """Ids in range (the device kernels do not bound-check), and the structure each case is
    named for."""
    for name in R.CASES:
        num_src, num_dst, src, dst = R.case(name)
        assert src.dtype == np.int64 and dst.dtype == np.int64 and src.shape == dst.shape
        if len(src):
            assert 0 <= src.min() and src.max() < num_src and 0 <= dst.min() and dst.max() < num_dst
    for n in R.BITS_N:
        _, _, src, dst = R.case("bits_n%d" % n)
        for ends in (src, dst):
            assert {0, max(n - 2, 0), n - 1, R.top_row_alias(n)} <= set(ends.tolist())
            # the top row and its alias interleave: neither's edges all come first
            if n >= 3:
                top, alias = np.flatnonzero(ends == n - 1), np.flatnonzero(ends == R.top_row_alias(n))
                assert top[0] < alias[-1] and alias[0] < top[-1]
    assert [R.top_row_alias(n) for n in (2, 3, 256, 257, 65536)] == [0, 0, 127, 0, 32767]
    assert [len(R.case("empty_n%d" % n)[2]) for n in (0, 1, 7)] == [0, 0, 0]
    for w in ("first", "middle", "last"):
        n, _, src, _ = R.case("one_row_" + w)
        assert len(src) == 5000 and len(set(src.tolist())) == 1
        assert src[0] == {"first": 0, "middle": n // 2, "last": n - 1}[w]
    n, _, src, dst = R.case("wide_2p20_rows")
    assert n == 1 << 20 and len(src) == 5
    n, _, src, _ = R.case("gap_100k_empty_rows")
    rows = np.unique(src)
    assert len(rows) == 2 and rows[1] - rows[0] - 1 >= 100_000 and rows[0] > 0 and rows[1] < n - 1
    n, _, src, dst = R.case("parallel_edges")
    assert len(src) == 3000 and len(np.unique(src * n + dst)) <= 40
    for name, nnz, longest in (("seam_300", 300, 100), ("seam_6000", 6000, 1900)):
        n, _, src, _ = R.case(name)
        deg = np.bincount(src, minlength=n)
        assert len(src) == nnz and deg.max() >= longest and (deg == 0).sum() > 5
        assert deg[0] == 0 and deg[-1] == 0
        # interleaved: the long row has edges in every 64th of the list
        long_row = int(deg.argmax())
        parts = np.array_split(src == long_row, 64 if nnz > 300 else 16)
        assert all(p.any() for p in parts)


def _ws64(n, nnz):
    return int(_ffi.lib().DGLMICOOToCSRDevice64WorkspaceBytes(n, nnz))


# (num_rows, nnz) -> DGLMICOOToCSRDevice64WorkspaceBytes of the commit before the batch
# length became a run-time value.  The size holds the scratch of the radix sort and the
# scans, which hipCUB reports per device: 0 bytes where it finds none
WS64_BEFORE = {
    (10, 0): {False: 256, True: 256},
    (3000, 40000): {False: 664064, True: 984064},
    (1 << 22, (1 << 31) + (1 << 20) + 3): {False: 17213423872, True: 25870471680},
}


@pytest.mark.parametrize("shape", sorted(WS64_BEFORE))
def test_workspace_bytes_unchanged_without_the_knob(shape, monkeypatch):
    monkeypatch.delenv("DGLMI_INGEST_BATCH", raising=False)
    assert _ws64(*shape) == WS64_BEFORE[shape][th.cuda.is_available()]


def test_ingest_batch_knob_parsing(monkeypatch):
    """An integer in [1, 2^30] is taken, on every call; anything else is ignored."""
    n, nnz = 3000, 40000
    monkeypatch.delenv("DGLMI_INGEST_BATCH", raising=False)
    default = _ws64(n, nnz)
    big = _ws64(1 << 22, (1 << 31) + 5)
    for junk in ("", "abc", "0", "-5", "12x", "1.5", " ", str((1 << 30) + 1), "9" * 30):
        monkeypatch.setenv("DGLMI_INGEST_BATCH", junk)
        assert _ws64(n, nnz) == default, junk
        assert _ws64(1 << 22, (1 << 31) + 5) == big, junk
    monkeypatch.setenv("DGLMI_INGEST_BATCH", str(1 << 30))
    assert _ws64(1 << 22, (1 << 31) + 5) == big
    sizes = []
    for b in (1, 1000, nnz - 1, nnz, nnz + 1):
        monkeypatch.setenv("DGLMI_INGEST_BATCH", str(b))
        sizes.append(_ws64(n, nnz))
        assert _ws64(n, 0) == 256
    assert sizes[0] < sizes[1] < sizes[2] <= sizes[3] == sizes[4] == default
    # four int32 arrays of one batch + the per-row cursor, each rounded up to 256 bytes
    fixed = -(-(n + 1) * 8 // 256) * 256
    assert sizes[1] >= fixed + 4 * (-(-1000 * 4 // 256) * 256)
    monkeypatch.delenv("DGLMI_INGEST_BATCH")
    assert _ws64(n, nnz) == default
