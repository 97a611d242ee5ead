"""Hub plans (DGLMIGraph.{in,out}_hub_plan): the copy_u sum whose hub rows' edges are
sorted by source block and reduced into per-block partial rows, merged in block order.
Small graphs with the gates lowered (n = 4,096, about 60 K edges, hubs from degree 8):
at this size a chunk is 8 positions, a workgroup 128 (F = 64) or 64 (F = 128).
Forward (in-CSR plan) and source gradient (out-CSR plan) against the fp64 index_add_
restatement within test_hints_gpu's bound 1e-4 + 1e-6 * mass; two calls bit-equal;
cold marks on and off bit-equal; one graph per structural case, each also mirrored so
both walks see it."""
import pytest
import torch as th

from dgl import kernel as K
from dgl.graph_index import ImmutableGraphIndex, device_block_gidx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 4096
FEATS = (64, 128)


@pytest.fixture(autouse=True)
def gates(monkeypatch):
    monkeypatch.delenv("DGLMI_HUB_DEGREE", raising=False)
    monkeypatch.delenv("DGLMI_HUB_HOT_DEGREE", raising=False)
    monkeypatch.delenv("DGLMI_HOT_DEGREE", raising=False)
    monkeypatch.setattr(ImmutableGraphIndex, "HUB_DEGREE", 8)
    monkeypatch.setattr(ImmutableGraphIndex, "HUB_MIN_TABLE_BYTES", 0)
    monkeypatch.setattr(ImmutableGraphIndex, "HUB_MIN_EDGE_SHARE", 0.0)
    monkeypatch.setattr(ImmutableGraphIndex, "HUB_MAX_PARTIAL_SHARE", 1e9)
    monkeypatch.setattr(ImmutableGraphIndex, "HOT_DEGREE", 0)  # marks: off unless a test asks
    monkeypatch.setattr(ImmutableGraphIndex, "HUB_HOT_DEGREE", None)


def _gen(seed):
    return th.Generator(device=DEV).manual_seed(seed)


def _skewed(m, seed, lo=0, hi=N):
    w = th.arange(1, hi - lo + 1, device=DEV, dtype=th.float32).pow(-0.9)
    return (th.multinomial(w, m, replacement=True, generator=_gen(seed)) + lo).to(th.int32)


def _uniform(m, seed, lo=0, hi=N):
    return th.randint(lo, hi, (m,), device=DEV, generator=_gen(seed), dtype=th.int32)


def _cat(*parts):
    return th.cat([p.to(th.int32) for p in parts])


def case_skewed():
    """test_hints_gpu's shape: skewed sources and (flipped) skewed destinations."""
    return _skewed(60_000, 1), (N - 1 - _skewed(60_000, 2)).to(th.int32)


def case_all_hubs():
    """Every non-empty row is a hub: 1,024 rows of 58-59 edges, the light part empty."""
    m = 60_000
    return _uniform(m, 3), (th.arange(m, device=DEV) % 1024).to(th.int32)


def case_star():
    """One row of 6,000 in-edges (750 chunks: whichever way its sources fall into blocks,
    some virtual row crosses more than 32 chunks -- the segmented fixup) among
    ordinary rows."""
    return (_cat(_uniform(6_000, 4), _uniform(54_000, 5)),
            _cat(th.full((6_000,), 777, device=DEV), _skewed(54_000, 6)))


def case_one_source_range():
    """Hub edges from three source ids only: at least five source blocks hold no edge."""
    src = th.tensor([5, 6, 4000], device=DEV)[_uniform(60_000, 7, 0, 3).long()]
    return src.to(th.int32), _skewed(60_000, 8)


def case_empty_runs():
    """Leading, middle and trailing runs of empty rows."""
    d = _skewed(60_000, 9, 0, 2000)
    return _uniform(60_000, 10), th.where(d < 1000, d + 500, d + 1500).to(th.int32)


def case_tiny_hub_part():
    """10 hubs of 50 edges: 500 hub positions, fewer than 8 workgroups (no remap); the
    other rows have at most 7 edges."""
    light = (th.arange(4 * N, device=DEV) % (N - 10) + 10).to(th.int32)
    hub = (th.arange(500, device=DEV) % 10).to(th.int32)
    return _uniform(500 + 4 * N, 11), _cat(hub, light)


def case_remainder():
    """2,725 hub positions (25 hubs of 109): 21 workgroups of 128 / 42 of 64 -- 16 / 40
    remapped, the others linear."""
    light = (th.arange(4 * N, device=DEV) % (N - 25) + 25).to(th.int32)
    hub = (th.arange(2725, device=DEV) % 25).to(th.int32)
    return _uniform(2725 + 4 * N, 12), _cat(hub, light)


CASES = {f.__name__[5:]: f for f in (case_skewed, case_all_hubs, case_star, case_one_source_range,
                                     case_empty_runs, case_tiny_hub_part, case_remainder)}


def _prime(g):
    """Build the hints and both plans now, under the class attributes of this moment."""
    g.gather_cols()
    g.hub_plan("in", 64)
    g.hub_plan("out", 64)
    return g


def _inputs(f, seed):
    x = th.rand(N, f, device=DEV, generator=_gen(seed)) * 2 - 1
    go = th.rand(N, f, device=DEV, generator=_gen(seed + 1)) * 2 - 1
    return x, go


def _run(g, x, go):
    out, gx = th.empty_like(x), th.empty_like(x)
    K.copy_reduce("sum", g, 0, x, out)
    K.backward_copy_reduce("sum", g, 0, x, out, go, gx)
    return out, gx


def _close(got, rows, cols, table):
    """got[r] == sum over positions of table[cols] within 1e-4 + 1e-6 * mass, in fp64."""
    t = table.double()[cols.long()]
    ref = th.zeros(N, table.shape[1], dtype=th.float64, device=DEV).index_add_(0, rows.long(), t)
    mass = th.zeros_like(ref).index_add_(0, rows.long(), t.abs())
    err = (got.double() - ref).abs()
    print("max err %.3e, bound at it %.3e" % (float(err.max()), float((1e-4 + 1e-6 * mass).flatten()[err.argmax()])))
    return bool((err <= 1e-4 + 1e-6 * mass).all())


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_planned_sum_and_source_gradient(case, reverse):
    src, dst = CASES[case]()
    if reverse:
        src, dst = dst, src
    g = device_block_gidx(N, N, src, dst)
    for f in FEATS:
        x, go = _inputs(f, 100)
        out, gx = _run(g, x, go)
        assert g._hub_plans["in"] is not None and g._hub_plans["out"] is not None
        assert _close(out, dst, src, x)
        assert _close(gx, src, dst, go)
        out2, gx2 = _run(g, x, go)
        assert th.equal(out, out2) and th.equal(gx, gx2)
    plan = g._hub_plans["out" if reverse else "in"]
    wg = {c: plan.hub_nnz // 8 // c for c in (16, 8)}  # workgroups of 16 / 8 chunks
    if case == "tiny_hub_part":
        assert plan.num_hubs == 10 and wg[16] < 8 and wg[8] < 8
    if case == "remainder":
        assert plan.hub_nnz == 2725 and wg[16] % 8 and wg[8] % 8
    if case == "all_hubs":
        assert plan.hub_nnz == plan.nnz and plan.num_hubs == 1024


def test_star_row_is_segmented_on_a_virtual_row():
    src, dst = case_star()
    g = device_block_gidx(N, N, src, dst)
    assert g.hub_plan("in", 64) is not None
    ptr = g._hub_plans["in"]._keep[3]
    virt = 8 * g._hub_plans["in"].num_hubs
    assert int((ptr[1:virt + 1] - ptr[:virt]).max()) > 33 * 8  # > kFixSeg continuation chunks


def test_empty_source_blocks():
    src, dst = case_one_source_range()
    g = device_block_gidx(N, N, src, dst)
    p = g.hub_plan("in", 64)
    ptr = g._hub_plans["in"]._keep[3].long()
    per_block = ptr[0:8 * p.num_hubs + 1:p.num_hubs]
    assert int(((per_block[1:] - per_block[:-1]) == 0).sum()) >= 5


def test_no_hub_row_builds_no_plan(monkeypatch):
    m = 6 * N
    src, dst = _uniform(m, 13), (th.arange(m, device=DEV) % N).to(th.int32)  # every in-degree 6
    g = device_block_gidx(N, N, src, dst)
    x, go = _inputs(64, 200)
    out, _ = _run(g, x, go)
    assert g._hub_plans["in"] is None
    monkeypatch.setattr(ImmutableGraphIndex, "HUB_DEGREE", 0)
    g0 = device_block_gidx(N, N, src, dst)
    out0, _ = _run(g0, x, go)
    assert g0._hub_plans == {"in": None, "out": None}
    assert th.equal(out, out0)


def test_marks_on_and_off_bit_equal(monkeypatch):
    src, dst = case_skewed()
    g0 = _prime(device_block_gidx(N, N, src, dst))
    monkeypatch.setattr(ImmutableGraphIndex, "HOT_DEGREE", 16)
    monkeypatch.setattr(ImmutableGraphIndex, "MIN_HINT_NODES", 0)
    monkeypatch.setattr(ImmutableGraphIndex, "MIN_HINT_EDGES", 0)
    monkeypatch.setattr(ImmutableGraphIndex, "MAX_COLD_SHARE", 1.0)
    gm = _prime(device_block_gidx(N, N, src, dst))
    monkeypatch.setattr(ImmutableGraphIndex, "HUB_HOT_DEGREE", 4)
    gm2 = _prime(device_block_gidx(N, N, src, dst))
    for f in FEATS:
        x, go = _inputs(f, 300)
        a, b, c = _run(g0, x, go), _run(gm, x, go), _run(gm2, x, go)
        assert th.equal(a[0], b[0]) and th.equal(a[1], b[1])
        assert th.equal(a[0], c[0]) and th.equal(a[1], c[1])
    assert g0._hub_plans["in"].marked is None and g0._hub_plans["out"].marked is None
    for g in (gm, gm2):
        for d in ("in", "out"):
            marked, cols = g._hub_plans[d]._keep[2], g._hub_plans[d]._keep[1]
            assert g._hub_plans[d].marked and 0.0 < float((marked < 0).float().mean()) < 1.0
            assert th.equal(marked & 0x7FFFFFFF, cols)
    # the hub part's own threshold marks fewer rows cold there
    h = gm._hub_plans["in"].hub_nnz
    assert int((gm2._hub_plans["in"]._keep[2][:h] < 0).sum()) < int((gm._hub_plans["in"]._keep[2][:h] < 0).sum())
    assert th.equal(gm2._hub_plans["in"]._keep[2][h:], gm._hub_plans["in"]._keep[2][h:])


def test_epilogue_launch_keeps_the_unplanned_path(monkeypatch):
    src, dst = case_skewed()
    g = device_block_gidx(N, N, src, dst)
    x, go = _inputs(64, 400)
    _run(g, x, go)
    assert g._hub_plans["in"] is not None
    monkeypatch.setattr(ImmutableGraphIndex, "HUB_DEGREE", 0)
    g0 = device_block_gidx(N, N, src, dst)
    row_mul = th.rand(N, device=DEV, generator=_gen(401))
    bias = th.randn(64, device=DEV, generator=_gen(402))
    oe, oe0 = th.empty_like(x), th.empty_like(x)
    K.copy_reduce("sum", g, 0, x, oe, epilogue=(row_mul, None, bias))
    K.copy_reduce("sum", g0, 0, x, oe0, epilogue=(row_mul, None, bias))
    assert g0.hub_plan("in", 64) is None
    assert th.equal(oe, oe0)
    # while the plain launch did take the plan: hub rows are summed block by block, in
    # another order than the unplanned walk's, so some of 4,096 x 64 sums differ in bits
    o, o0 = th.empty_like(x), th.empty_like(x)
    K.copy_reduce("sum", g, 0, x, o)
    K.copy_reduce("sum", g0, 0, x, o0)
    assert not th.equal(o, o0) and th.allclose(o, o0, rtol=1e-4, atol=1e-4)
