"""A numpy restatement of the graph ingest (csrc/ingest.hip: COO -> CSR, row expansion,
the in / out CSR pair of a block), for the tests of the device ingest.  It shares no code
with the library: every array comes from ``np.argsort(kind="stable")``, ``np.bincount``
and ``np.cumsum`` over the edge list, after the description of
``dgl.graph_index.device_block_gidx``:

    out-CSR = stable sort of the eid-ordered COO by src; in-CSR = stable re-sort of that
    sequence by dst, so every dst row lists its sources ascending, eids ascending within
    a source.

All arrays are int64; the tests cast them to the width of the entry they check.
tests/test_ingest_ref_cpu.py checks this file against the host COOToCSR / CSRTranspose
(pinned to the original project's answers in tests/test_host_cpu.py) on the case list
below, which tests/test_ingest_gpu.py then runs through the device entries.
"""
import numpy as np


def coo_to_csr(num_rows, row, col, data=None):
    """(indptr, indices, data) of the COO sorted by row, stably: within a row the
    positions of the COO ascend.  ``data`` defaults to the COO position (the edge id)."""
    row = np.asarray(row, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    order = np.argsort(row, kind="stable")
    indptr = np.zeros(num_rows + 1, np.int64)
    indptr[1:] = np.cumsum(np.bincount(row, minlength=num_rows))
    out = order.astype(np.int64) if data is None else np.asarray(data, dtype=np.int64)[order]
    return indptr, col[order], out


def expand_rows(indptr):
    """Row id of every CSR position: the number of rows 1 .. n-1 that start at or before
    it (an empty row starts where the next one does and is counted with it)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    nnz = int(indptr[-1])
    opened = np.bincount(indptr[1:-1], minlength=nnz + 1)[:nnz]
    return np.cumsum(opened).astype(np.int64)


def block(num_src, num_dst, src, dst):
    """(in_csr, out_csr) of a num_src -> num_dst block, each (indptr, indices, data, rows)."""
    o_ptr, o_idx, o_dat = coo_to_csr(num_src, src, dst)
    o_rows = expand_rows(o_ptr)
    i_ptr, i_idx, i_dat = coo_to_csr(num_dst, o_idx, o_rows, o_dat)
    return (i_ptr, i_idx, i_dat, expand_rows(i_ptr)), (o_ptr, o_idx, o_dat, o_rows)


# ---- the shared cases: name -> (num_src, num_dst, src, dst), int64, every id in range ----

# csrc/ingest.hip grid_of: at most 16384 blocks of 256 lanes, so 16384 * 256 items fill the
# first iteration of every grid-stride loop; three more reach the second
GRID_CAP_ITEMS = 16384 * 256
GRID_TAIL_NNZ = GRID_CAP_ITEMS + 3

# row counts on and around powers of two: the radix sort's key width (bits_for)
BITS_N = (1, 2, 3, 4, 5, 255, 256, 257, 65535, 65536, 65537)


def _shuffled(rs, src, dst):
    p = rs.permutation(len(src))
    return np.asarray(src, np.int64)[p], np.asarray(dst, np.int64)[p]


def top_row_alias(n):
    """The row that the top row n-1 sorts as when the highest bit of its id is dropped."""
    return (n - 1) - (1 << ((n - 1).bit_length() - 1)) if n >= 2 else 0


def _bits(n):
    """A few hundred random edges on n nodes plus edges that start and end in rows 0,
    n-2 and n-1 (the top row is the one a sort of one key bit too few misplaces) and in
    the top row's alias: the 64-bit path places every run of equal sorted keys at its
    row's cursor, so a mis-sort shows there only when the top row's edges interleave with
    those of the row it is taken for."""
    rs = np.random.RandomState(1000 + n)
    ends = sorted({0, max(n - 2, 0), n - 1, top_row_alias(n)})
    src = list(rs.randint(0, n, 300)) + [a for a in ends for _ in ends] * 3
    dst = list(rs.randint(0, n, 300)) + [b for _ in ends for b in ends] * 3
    return (n, n) + _shuffled(rs, src, dst)


def _empty(n):
    return n, n, np.empty(0, np.int64), np.empty(0, np.int64)


def _one_row(where):
    """5000 edges that all leave one row (first, middle or last of 301): every other row
    of the out-CSR is empty, and the in-CSR's rows are runs of parallel edges."""
    n = 301
    r = {"first": 0, "middle": 150, "last": n - 1}[where]
    rs = np.random.RandomState(7 + r)
    return n, n, np.full(5000, r, np.int64), rs.randint(0, n, 5000).astype(np.int64)


def _wide():
    n = 1 << 20
    src = np.array([n - 1, 0, n // 2, 1, n - 2], np.int64)
    dst = np.array([0, n - 1, n // 2, n - 2, n - 1], np.int64)
    return n, n, src, dst


def _gap():
    """Two populated rows with 100 000 empty ones between, and empty rows before and after."""
    lo, hi = 3, 100_004
    n = hi + 6
    rs = np.random.RandomState(11)
    ends = np.array([lo, hi], np.int64)
    return n, n, ends[rs.randint(0, 2, 400)], ends[rs.randint(0, 2, 400)]


def _parallel():
    """3000 edges over 40 (src, dst) pairs: sort stability, edge ids ascending in a pair."""
    n = 50
    rs = np.random.RandomState(13)
    pairs = np.stack([rs.randint(0, n, 40), rs.randint(0, n, 40)], 1).astype(np.int64)
    pick = rs.randint(0, 40, 3000)
    return n, n, pairs[pick, 0], pairs[pick, 1]


def _rect(num_src, num_dst):
    rs = np.random.RandomState(17 * num_src + num_dst)
    return (num_src, num_dst, rs.randint(0, num_src, 600).astype(np.int64),
            rs.randint(0, num_dst, 600).astype(np.int64))


def seam_degrees(nnz_small, seed):
    """Row degrees like tests/test_softmax_owned_gpu.py _degrees: many rows of 0 to 3
    edges, a few of a few hundred and one long one (scaled down for ``nnz_small``)."""
    rs = np.random.RandomState(seed)
    if nnz_small:
        deg, total = list(rs.randint(0, 4, 60)) + [40, 55], 300
    else:
        deg, total = list(rs.randint(0, 4, 1200)) + list(rs.randint(200, 400, 7)), 6000
    deg.append(total - 1 - sum(deg))  # the long row: about 110 / about 2000 edges
    deg = [0, 0] + deg + [0, 1, 0]  # empty rows at both ends
    body = deg[2:-3]
    rs.shuffle(body)
    deg[2:-3] = body
    return np.array(deg, np.int64)


def _seam(nnz_small):
    """Rows of very different lengths, the edges in an order that interleaves the rows over
    the whole list: every batch of the 64-bit sort holds a piece of the long rows, so a
    row is filled from many batches."""
    deg = seam_degrees(nnz_small, 23)
    n = len(deg)
    rs = np.random.RandomState(29)
    src = np.repeat(np.arange(n, dtype=np.int64), deg)
    dst = rs.randint(0, n, len(src)).astype(np.int64)
    return (n, n) + _shuffled(rs, src, dst)


def grid_tail():
    """GRID_TAIL_NNZ edges on 1000 nodes (about 4200 per row): every grid-stride loop of
    the ingest kernels takes a second iteration."""
    rs = np.random.RandomState(31)
    n = 1000
    return (n, n, rs.randint(0, n, GRID_TAIL_NNZ).astype(np.int64),
            rs.randint(0, n, GRID_TAIL_NNZ).astype(np.int64))


CASES = {}
for _n in BITS_N:
    CASES["bits_n%d" % _n] = (_bits, (_n,))
for _n in (0, 1, 7):
    CASES["empty_n%d" % _n] = (_empty, (_n,))
CASES["one_edge_n1"] = (lambda: (1, 1, np.zeros(1, np.int64), np.zeros(1, np.int64)), ())
CASES["one_edge_n7"] = (lambda: (7, 7, np.array([3], np.int64), np.array([5], np.int64)), ())
for _w in ("first", "middle", "last"):
    CASES["one_row_" + _w] = (_one_row, (_w,))
CASES["wide_2p20_rows"] = (_wide, ())
CASES["gap_100k_empty_rows"] = (_gap, ())
CASES["parallel_edges"] = (_parallel, ())
for _s, _d in ((1, 500), (500, 1), (37, 4100), (4100, 37)):
    CASES["rect_%dx%d" % (_s, _d)] = (_rect, (_s, _d))
CASES["seam_300"] = (_seam, (True,))
CASES["seam_6000"] = (_seam, (False,))


def case(name):
    fn, args = CASES[name]
    return fn(*args)


def edge_data(nnz, seed=37):
    """An explicit ``data`` argument: a random permutation of the edge ids."""
    return np.random.RandomState(seed).permutation(nnz).astype(np.int64)
