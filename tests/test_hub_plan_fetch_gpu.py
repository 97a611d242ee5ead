"""The hub plan's 16-lane walk (F = 36, 64) stages 32 positions per batch: one 8-byte
column load per lane, the batch's flags one whole word of the start bitmap, up to 32 window
entries of `row_ids`.  None of it may move a bit.  Small
graphs (n = 4,096, gates lowered as in test_hub_plan_rows_gpu) whose plans come from
`build_hub_plan` through `ImmutableGraphIndex.hub_plan` and reach the kernel through the C
entry.  The chunk size follows nnz (`fast_chunk_edges`: 8 positions below 2^18 edges, 16
below 2^19, 64 from 2^20, 512 from 2^23), so the cases pick their nnz: most carry 256 hubs
of 4,096 edges (2^20 hub positions, chunks of 64 = two batches; the light part then starts
on a chunk) and shape the light part, which keeps CSR order, position by position.

Every case runs forward on the in-CSR plan or mirrored (`reverse`) so that the source
gradient's out-CSR plan walks the same structure, with cold marks off (VAR 3) and on
(VAR 11), at F = 36 and 64 (one case at 128 as well: the 32-lane instance), and is held to

1. the SHA-256 of the output and the source gradient in
   tests/golden/hub_plan_fetch_sha.json, recorded by scripts/record_hub_plan_fetch_sha.py
   with a library built from the commit named in that file (before this walk);
2. two launches into NaN-filled buffers give equal bits;
3. the fp64 index_add_ restatement within 1e-4 + 1e-6 * mass (not `wide_chunks`, whose
   8.4 M edges make the restatement the slowest part by far; its bits are held by 1)."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch as th

from dgl import kernel as K
from dgl.graph_index import ImmutableGraphIndex, device_block_gidx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 4096
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hub_plan_fetch_sha.json")

GATES = {"HUB_MIN_TABLE_BYTES": 0, "HUB_MIN_EDGE_SHARE": 0.0, "HUB_MAX_PARTIAL_SHARE": 1e9,
         "HOT_DEGREE": 0, "HUB_HOT_DEGREE": None}
MARKS = {"HOT_DEGREE": 16, "MIN_HINT_NODES": 0, "MIN_HINT_EDGES": 0, "MAX_COLD_SHARE": 1.0}

HUB_DEGREE = 1024  # of the cases with big hubs: light rows have up to 1,023 edges


def _rows(light, hubs):
    """The row of every edge: `light` and `hubs` are (row, degree) lists."""
    pairs = list(light) + list(hubs)
    return np.repeat(np.array([r for r, _ in pairs], np.int64), np.array([d for _, d in pairs], np.int64))


def _big_hubs(first=N - 256, count=256):
    """`count` hubs of 4,096 edges: 2^20 positions when count = 256."""
    return [(first + k, 4096) for k in range(count)]


def _light(degs, first=0, step=1):
    """Consecutive light rows (ids first, first + step ..) of the given degrees."""
    return [(first + i * step, d) for i, d in enumerate(degs)]


def _tail(rem):
    """nnz = rem (mod 64): the last chunk holds `rem` positions."""
    degs = [3] * 400
    degs += [(-sum(degs)) % 64 + 64]  # whole chunks up to here
    degs += [d for d in (min(rem, 5), rem - min(rem, 5)) if d]
    rows = _rows(_light(degs), _big_hubs())
    assert rows.shape[0] % 64 == rem
    return HUB_DEGREE, rows


def case_tail_1():
    """Chunks of 64; the last chunk is one position: a batch of one."""
    return _tail(1)


def case_tail_33():
    """The last chunk ends one position into its second batch."""
    return _tail(33)


def case_tail_47():
    """The last chunk ends in the middle of its second batch, on an odd count: the last
    lane that loads anything loads one column, not two."""
    return _tail(47)


def case_degree_one_runs():
    """Runs of 100 and 70 rows of one edge (batches that start 32 rows: the window consumed
    whole, both entries of every lane), each followed by a row of 200 or 96 edges (batches
    that start none: no window load), at four alignments to the batch."""
    degs = []
    for shift in (0, 7, 16, 25):
        degs += ([shift] if shift else []) + [1] * 100 + [200] + [1] * 70 + [96]
        degs += [(-sum(degs)) % 32 + 32]
    return HUB_DEGREE, _rows(_light(degs), _big_hubs())


def case_word_positions():
    """Row starts at in-word positions 0, 15, 16, 17 and 31: all five in every word, then
    one per word -- rows of 32 edges shifted to start at 15, 16, 17, 31 and 0."""
    degs = [15, 1, 1, 14, 1] * 100
    for shift in (15, 1, 1, 14, 1):
        degs += [shift] + [32] * 50
    return HUB_DEGREE, _rows(_light(degs), _big_hubs())


def case_chunk_edges():
    """Rows that end exactly at a chunk's last position and rows that begin at a chunk's
    first (chunks of 64): whole-chunk rows, 40 + 24, 1 + 63, 10 + 54, and a row over two
    whole chunks, whose carry the fixup folds."""
    degs = [64, 40, 24, 1, 63, 10, 54, 128, 64, 63, 1, 32, 32, 192, 24, 40] * 20
    return HUB_DEGREE, _rows(_light(degs), _big_hubs())


def case_small_k8():
    """60,000 edges: chunks of 8 positions, each inside one bitmap word at shifts 0, 8, 16,
    24 -- one batch per chunk, loaded by the same 8-byte column loads.  A row of 6,000
    edges (virtual rows of more than 32 chunks) among skewed rows, most of one or a few
    edges."""
    rs = np.random.RandomState(33)
    rows = np.concatenate([np.full(6000, 777), np.arange(2000, 2080),
                           (rs.pareto(1.2, 53_920) * 50).astype(np.int64) % N])
    return 8, np.sort(rows, kind="stable")


def case_small_k16():
    """300,001 edges: chunks of 16 positions (shifts 0 and 16 in a word), an odd tail."""
    rs = np.random.RandomState(34)
    rows = np.concatenate([np.arange(1000, 1100), (rs.pareto(1.2, 299_901) * 50).astype(np.int64) % N])
    assert 2 ** 18 <= rows.shape[0] < 2 ** 19
    return 32, np.sort(rows, kind="stable")


def case_segmented():
    """A hub of 40,000 edges next to 246 of 4,096: its virtual row in each of the eight
    source blocks spans about 78 chunks of 64, more than the 32 continuation chunks one
    fixup group folds (the segmented fixup)."""
    degs = [(1, 5, 33, 64, 2)[i % 5] for i in range(500)]
    return HUB_DEGREE, _rows(_light(degs), [(N - 300, 40_000)] + _big_hubs(N - 246, 246))


def case_empty_rows():
    """Empty rows at the start (40), in the middle (runs of 1, 31, 32, 33 and 65 between
    light rows; the hubs sit in the middle too) and at the end (the last 500)."""
    light, r = [], 40
    for i in range(15):
        for gap in (1, 31, 32, 33, 65):
            if 1500 <= r < 1800:
                r = 1800
            light.append((r, 1 + (i * 7 + gap) % 40))
            r += gap + 1
    assert r < N - 500
    return HUB_DEGREE, _rows(light, _big_hubs(1500, 256))


def case_wide_chunks():
    """2,048 hubs of 4,096 edges (2^23 positions): chunks of 512, sixteen batches and
    sixteen bitmap words each, so the batch's word index and the window index run on."""
    degs = [(1, 1, 1, 40, 600, 7, 32, 31, 33)[i % 9] for i in range(900)]
    rows = _rows(_light(degs), _big_hubs(N - 2048, 2048))
    assert rows.shape[0] >= 2 ** 23
    return HUB_DEGREE, rows


CASES = {f.__name__[5:]: f for f in (
    case_tail_1, case_tail_33, case_tail_47, case_degree_one_runs, case_word_positions,
    case_chunk_edges, case_small_k8, case_small_k16, case_segmented, case_empty_rows,
    case_wide_chunks)}
# chunk size each case is built for (fast_chunk_edges of its nnz)
CHUNK = {"small_k8": 8, "small_k16": 16, "wide_chunks": 512}
NO_RESTATEMENT = ("wide_chunks",)


def feats(case):
    return (36, 64, 128) if case == "degree_one_runs" else (36, 64)


def chunk_edges(nnz):
    """fast_chunk_edges for rows of 16 floats or more (kernels_spmm.hip)."""
    k = 512
    while k > 8 and nnz // k < 256 * 64:
        k >>= 1
    return k


def set_gates(setter, hub_degree, marks):
    """`setter(name, value)` sets an ImmutableGraphIndex class attribute."""
    for k, v in GATES.items():
        setter(k, v)
    setter("HUB_DEGREE", hub_degree)
    if marks:
        for k, v in MARKS.items():
            setter(k, v)


def case_graph(case):
    """(hub degree, rows, cols) of the walk under test, as device int32: the in-CSR's rows
    and sources, or mirrored the out-CSR's rows and destinations."""
    deg, rows = CASES[case]()
    cols = np.random.RandomState(len(case) + 7 * rows.shape[0]).randint(0, N, rows.shape[0])
    t = lambda a: th.from_numpy(a.astype(np.int32)).to(DEV)
    return deg, t(rows), t(cols)


def run_case(g, f):
    """Output and source gradient (NaN-filled first) of the planned sum at width f."""
    rs = np.random.RandomState(1000 + f)
    x = th.from_numpy(rs.uniform(-1, 1, (N, f)).astype(np.float32)).to(DEV)
    go = th.from_numpy(rs.uniform(-1, 1, (N, f)).astype(np.float32)).to(DEV)
    out, gx = th.full_like(x, float("nan")), th.full_like(x, float("nan"))
    K.copy_reduce("sum", g, 0, x, out)
    K.backward_copy_reduce("sum", g, 0, x, out, go, gx)
    return x, go, out, gx


def digest(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def key(case, reverse, f):
    return "%s-%s-%d" % (case, "out" if reverse else "in", f)


def _close(got, rows, cols, table):
    t = table.double()[cols.long()]
    ref = th.zeros(N, table.shape[1], dtype=th.float64, device=DEV).index_add_(0, rows.long(), t)
    mass = th.zeros_like(ref).index_add_(0, rows.long(), t.abs())
    err = (got.double() - ref).abs()  # a NaN left in `got` fails the comparison below
    print("max err %.3e" % float(err.nan_to_num(float("inf")).max()))
    return bool((err <= 1e-4 + 1e-6 * mass).all())


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)["digests"]


def test_cases_are_what_they_say():
    """The structure each case promises, read from the rows alone (no launch)."""
    for case, make in CASES.items():
        deg, rows = make()
        assert rows.min() >= 0 and rows.max() < N
        assert chunk_edges(rows.shape[0]) == CHUNK.get(case, 64), case
        d = np.bincount(rows, minlength=N)
        hub_nnz = int(d[d >= deg].sum())
        assert hub_nnz > 0
        if case not in CHUNK:
            assert hub_nnz % 64 == 0  # the light part starts on a chunk
    _, rows = CASES["degree_one_runs"]()
    d = np.bincount(rows, minlength=N)
    one = "".join("1" if x == 1 else "0" for x in d[:1000])
    assert "1" * 64 in one
    _, rows = CASES["empty_rows"]()
    d = np.bincount(rows, minlength=N)
    assert (d[:40] == 0).all() and (d[-500:] == 0).all() and (d[40:-500] == 0).any()
    _, rows = CASES["segmented"]()
    assert np.bincount(rows).max() // 8 > 33 * 64
    for rem in (1, 33, 47):
        assert CASES["tail_%d" % rem]()[1].shape[0] % 64 == rem


@pytest.mark.parametrize("marks", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_plan_walk_keeps_the_parents_bits(case, reverse, marks, monkeypatch, golden):
    for name in ("DGLMI_HUB_DEGREE", "DGLMI_HUB_HOT_DEGREE", "DGLMI_HOT_DEGREE"):
        monkeypatch.delenv(name, raising=False)
    deg, rows, cols = case_graph(case)
    set_gates(lambda k, v: monkeypatch.setattr(ImmutableGraphIndex, k, v), deg, marks)
    src, dst = (rows, cols) if reverse else (cols, rows)
    g = device_block_gidx(N, N, src, dst)
    walk = "out" if reverse else "in"
    for f in feats(case):
        x, go, out, gx = run_case(g, f)
        plan = g._hub_plans[walk]
        assert plan is not None and bool(plan.marked) == marks
        _, _, out2, gx2 = run_case(g, f)
        assert th.equal(out, out2) and th.equal(gx, gx2)
        want = golden[key(case, reverse, f)]
        assert digest(out) == want["out"] and digest(gx) == want["grad"]
        if case not in NO_RESTATEMENT:
            assert _close(out, dst, src, x)
            assert _close(gx, src, dst, go)
    # the walk under test saw the rows the case describes
    assert plan.nnz == rows.shape[0]
    ids = plan._keep[7]
    assert th.equal(ids.long(), th.unique_consecutive(plan._keep[0].long()))
