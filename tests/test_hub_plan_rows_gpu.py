"""The hub plan's walk reads its row starts from a bitmap and a list of row ids
(DGLMIHubPlan.starts / start_rank / row_ids) instead of one row id per position.  Small
graphs (n = 4,096) with the gates lowered as in test_hub_plan_gpu, built so that row starts
fall where the walk's batches (16 / 32 / 64 positions at F = 64 / 128 / 256), its chunks
(8 positions at this size; 64 in `long_chunks`) and the bitmap's 32-bit words meet.  Each
case runs forward on the in-CSR plan, or mirrored (`reverse`) so that the source gradient's
out-CSR plan walks the same structure, with cold marks off and on, and is held to

1. the fp64 index_add_ restatement within 1e-4 + 1e-6 * mass, the output buffers filled
   with NaN beforehand;
2. two calls give equal bits;
3. the bits are those of the walk that read `rows`: SHA-256 of the output and the source
   gradient in tests/golden/hub_plan_rows_sha.json, recorded by
   scripts/record_hub_plan_rows_sha.py against a library built before the change."""
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
FEATS = (64, 128, 256)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hub_plan_rows_sha.json")

# test_hub_plan_gpu's gates; HUB_DEGREE is each case's own
GATES = {"HUB_MIN_TABLE_BYTES": 0, "HUB_MIN_EDGE_SHARE": 0.0, "HUB_MAX_PARTIAL_SHARE": 1e9,
         "HOT_DEGREE": 0, "HUB_HOT_DEGREE": None}
MARKS = {"HOT_DEGREE": 16, "MIN_HINT_NODES": 0, "MIN_HINT_EDGES": 0, "MAX_COLD_SHARE": 1.0}


def _rows(light, hubs):
    """The row of every edge: `light` and `hubs` are (row, degree) lists."""
    pairs = list(light) + list(hubs)
    return np.repeat(np.array([r for r, _ in pairs], np.int64), np.array([d for _, d in pairs], np.int64))


# four hubs of 64 edges on the last rows: the hub part is 256 positions, so the light part,
# which follows it in CSR order, starts on a word of the bitmap
HUBS = [(N - 4 + k, 64) for k in range(4)]


def case_degree_one():
    """3,000 light rows of one edge: 16 starts in every batch, the window consumed whole."""
    return 8, _rows([(r, 1) for r in range(3000)], HUBS)


def case_degrees_15_16_17():
    """Light rows of 15, 16, 17 edges end to end, then 17, 16, 15: starts on, just before
    and just after the batch boundaries."""
    degs = [(15, 16, 17)[i % 3] for i in range(300)] + [(17, 16, 15)[i % 3] for i in range(300)]
    return 32, _rows(list(enumerate(degs)), HUBS)


def case_degrees_8_24():
    """Light rows of 8, 24, 8, 24 .. edges, then 24, 8, 24, 8 ..: 8-position chunks begin on
    a start and in the middle of a row, among them the chunks at base % 32 == 24, whose
    batch straddles two bitmap words -- with a start at its first position or not."""
    degs = [(8, 24)[i % 2] for i in range(200)] + [(24, 8)[i % 2] for i in range(200)]
    return 32, _rows(list(enumerate(degs)), HUBS)


def case_empty_runs():
    """Runs of 1, 31, 32 and 33 empty rows between non-empty ones: row ids jump."""
    light, r = [], 0
    for i in range(40):
        for gap in (1, 31, 32, 33):
            light.append((r, 1 + (i + gap) % 5))
            r += gap + 1
    assert r < N - 4
    return 8, _rows(light, HUBS)


def _tail(rem):
    light = [(r, 2) for r in range(200)]
    light += [(1000 + k, d) for k, d in enumerate((min(rem, 5), rem - min(rem, 5))) if d]
    rows = _rows(light, HUBS)
    assert rows.shape[0] % 16 == rem
    return 8, rows


def case_tail_1():
    """nnz = 1 (mod 16): the last batch holds one position."""
    return _tail(1)


def case_tail_7():
    return _tail(7)


def case_tail_9():
    return _tail(9)


def case_star():
    """A row of 6,000 edges among skewed rows: a virtual row of more than 32 chunks."""
    rs = np.random.RandomState(21)
    return 8, np.concatenate([np.full(6000, 777), (rs.pareto(1.2, 54_000) * 50).astype(np.int64) % N])


def case_all_hubs():
    """1,024 rows of 58-59 edges and no other: the light part is empty."""
    return 8, np.arange(60_000, dtype=np.int64) % 1024


def case_long_chunks():
    """1.1 M edges: chunks of 64 positions, four (F = 64), two or one batch each, so the
    window index runs on from batch to batch; 256 hubs of 4,096 edges (their virtual rows
    span about eight chunks) and light rows of 1 .. 40 edges."""
    return 1024, _rows([(r, 1 + r % 40) for r in range(3000)], [(N - 256 + k, 4096) for k in range(256)])


CASES = {f.__name__[5:]: f for f in (
    case_degree_one, case_degrees_15_16_17, case_degrees_8_24, case_empty_runs, case_tail_1,
    case_tail_7, case_tail_9, case_star, case_all_hubs, case_long_chunks)}


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


def run_case(g, reverse, f):
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
        return json.load(fh)


@pytest.mark.parametrize("marks", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_row_starts_from_the_bitmap(case, reverse, marks, monkeypatch, golden):
    for name in ("DGLMI_HUB_DEGREE", "DGLMI_HUB_HOT_DEGREE", "DGLMI_HOT_DEGREE"):
        monkeypatch.delenv(name, raising=False)
    deg, rows, cols = case_graph(case)
    set_gates(lambda k, v: monkeypatch.setattr(ImmutableGraphIndex, k, v), deg, marks)
    src, dst = (rows, cols) if reverse else (cols, rows)
    g = device_block_gidx(N, N, src, dst)
    walk = "out" if reverse else "in"
    for f in FEATS:
        x, go, out, gx = run_case(g, reverse, f)
        plan = g._hub_plans[walk]
        assert plan is not None and bool(plan.marked) == marks
        assert _close(out, dst, src, x)
        assert _close(gx, src, dst, go)
        _, _, out2, gx2 = run_case(g, reverse, f)
        assert th.equal(out, out2) and th.equal(gx, gx2)
        want = golden[key(case, reverse, f)]
        assert digest(out) == want["out"] and digest(gx) == want["grad"]
    if case == "all_hubs":
        assert plan.hub_nnz == plan.nnz
    if case == "long_chunks":
        assert plan.nnz >= 64 * 16384  # chunks of 64 positions (fast_chunk_edges)
    # the walk under test saw the rows the case describes
    ids = plan._keep[7]
    assert th.equal(ids.long(), th.unique_consecutive(plan._keep[0].long()))
