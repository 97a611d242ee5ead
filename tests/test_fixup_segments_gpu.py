"""Every instance of the segmented-fixup protocol (csrc/internal.h: fixup_role, seg_fold,
seg_reset) on one small graph whose hub rows sit on both sides of each segment boundary.

A row that starts on a chunk boundary and has K * c + 1 entries has exactly c continuation
chunks of K positions, so nseg = (c - 1 + kFixSeg) / kFixSeg with kFixSeg = 32: the hub
degrees K * c + 1 for K in {8, 16, 32, 64} and c in {1, 2, 32, 33, 64, 65} give nseg = 1, 1,
1, 2, 2, 3 at every chunk size in use, and one row of 8 * 1025 + 1 entries gives 33 segments
(more than kFixSeg: the last group's own fold is long).  Padding rows put every hub row's
start on a multiple of 64 positions ("aligned"); "shifted" has five more leading entries, so
no row starts on a boundary; "swapped" exchanges source and destination, so the out-CSR
walks (source gradients) see the hubs.  Edges are inserted in shuffled order: edge ids are
not positions, and the edge softmax takes its chunked walk.

Chunk sizes at this size (about 3.4 * 10^4 edges), by the rules at the time of writing:
K = 8 for the spmm, lane, generic and fused-GAT walks (fast_chunk_edges, gat_chunk_edges,
gat_bwd_chunk_edges), K = 64 / 32 / 16 for the edge softmax at H <= 4 / 8 / 16
(softmax_chunk_edges).  If those rules change, revisit the degree set.

References and bounds are those of the suite: fp64 torch within 1e-4 + 1e-6 * sum|terms| per
row for sums (test_hub_rows_gpu, test_blocks_gpu; scaled by the epilogue's row factor as in
test_kernels_gpu.test_fused_epilogue), exact equality for max / min, test_hub_rows_gpu's
tolerances for the fused GAT and the edge softmax; every case run twice is bit-equal.
scripts/fixup_ab.py runs the same cases (run_case) to compare two library builds bit by bit.
"""
import contextlib
import os

import numpy as np
import pytest
import torch as th

import dgl
import dgl.backend as B
import dgl.function as fn
from dgl import kernel as K
from dgl.graph_index import ImmutableGraphIndex, device_block_gidx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 512
VARIANTS = ("aligned", "shifted", "swapped")
HUB_DEGREES = [k * c + 1 for k in (8, 16, 32, 64) for c in (1, 2, 32, 33, 64, 65)] + [8 * 1025 + 1]


def hub_edges(variant):
    """(src, dst) int64 numpy: pad row 2i, hub row 2i + 1; rows from 2 * len(HUB_DEGREES) on
    have no in-edges."""
    rs = np.random.RandomState(7)
    deg = np.zeros(N, np.int64)
    lead = 5 if variant == "shifted" else 0  # row 0 gets them: every later start moves by five
    pos = 0
    for i, d in enumerate(HUB_DEGREES):
        deg[2 * i] = (lead - pos) % 64
        deg[2 * i + 1] = d
        pos += deg[2 * i] + d
    dst = np.repeat(np.arange(N), deg)
    src = rs.randint(0, N, dst.size)
    hub_start = np.cumsum(deg)[0:2 * len(HUB_DEGREES):2]
    assert (hub_start % 64 == lead).all() and dst.size < 10 ** 5
    perm = rs.permutation(dst.size)
    src, dst = src[perm], dst[perm]
    return (dst, src) if variant == "swapped" else (src, dst)


def _rand(seed, *shape, lo=-1.0, hi=1.0):
    """Fixed inputs drawn on the CPU (the same for every library build)."""
    x = np.random.RandomState(seed).uniform(lo, hi, shape).astype(np.float32)
    return th.from_numpy(x).to(DEV)


_GRAPHS = {}


def graph(variant):
    if variant not in _GRAPHS:
        src, dst = hub_edges(variant)
        g = dgl.DGLGraph()
        g.add_nodes(N)
        g.add_edges(src, dst)
        _GRAPHS[variant] = (g, th.from_numpy(src).to(DEV), th.from_numpy(dst).to(DEV))
    return _GRAPHS[variant]


@contextlib.contextmanager
def open_hub_gates():
    """The hub plan's gates as tests/test_hub_plan_gpu.py opens them."""
    names = {"HUB_DEGREE": 8, "HUB_MIN_TABLE_BYTES": 0, "HUB_MIN_EDGE_SHARE": 0.0,
             "HUB_MAX_PARTIAL_SHARE": 1e9, "HOT_DEGREE": 0, "HUB_HOT_DEGREE": None}
    env = {k: os.environ.pop(k, None) for k in ("DGLMI_HUB_DEGREE", "DGLMI_HUB_HOT_DEGREE", "DGLMI_HOT_DEGREE")}
    old = {k: getattr(ImmutableGraphIndex, k) for k in names}
    for k, v in names.items():
        setattr(ImmutableGraphIndex, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(ImmutableGraphIndex, k, v)
        os.environ.update({k: v for k, v in env.items() if v is not None})


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---- the cases: run(variant) -> {name: tensor}, check(variant, outputs) ------------------
def _sum_ref(rows, cols, table):
    t = table.double()[cols]
    exact = th.zeros((N,) + table.shape[1:], dtype=th.float64, device=DEV).index_add_(0, rows, t)
    mass = th.zeros_like(exact).index_add_(0, rows, t.abs())
    return exact, mass


def _sum_close(name, got, exact, mass, scale=1.0):
    err = (got.double() - exact).abs()
    bound = 1e-4 + 1e-6 * mass * scale
    print("%s: max err %.3e (bound there %.3e)" % (name, float(err.max()), float(bound.flatten()[err.argmax()])))
    assert (err <= bound).all(), name


def _run_sum(feat):
    def run(variant):
        g, _, _ = graph(variant)
        x = _rand(feat, N, feat).requires_grad_()
        g.ndata["x"] = x
        g.update_all(fn.copy_u("x", "m"), fn.sum("m", "h"))
        h = g.ndata["h"]
        (gx,) = th.autograd.grad(h, x, _rand(100 + feat, N, feat))
        return {"out": h.detach(), "grad_src": gx}

    def check(variant, o):
        _, s, d = graph(variant)
        _sum_close("out", o["out"], *_sum_ref(d, s, _rand(feat, N, feat)))
        # d/dx[u] = the sum over u's out-edges of grad_out[v]: the reverse graph's sum
        _sum_close("grad_src", o["grad_src"], *_sum_ref(s, d, _rand(100 + feat, N, feat)))
    return run, check


def _run_maxmin(red):
    def run(variant):
        g, _, _ = graph(variant)
        g.ndata["x"] = _rand(20, N, 64)
        g.update_all(fn.copy_u("x", "m"), getattr(fn, red)("m", "h"))
        return {"out": g.ndata["h"]}

    def check(variant, o):
        _, s, d = graph(variant)
        x = _rand(20, N, 64)
        ref = th.full((N, 64), float("-inf") if red == "max" else float("inf"), device=DEV)
        ref.index_reduce_(0, d, x[s], "amax" if red == "max" else "amin")
        has = th.bincount(d, minlength=N) > 0
        assert th.equal(o["out"][has], ref[has])
    return run, check


def _epi_run(variant):
    g, _, _ = graph(variant)
    out = th.empty(N, 64, device=DEV)
    K.copy_reduce("sum", g._graph.get_immutable_gidx(DEV), 0, _rand(30, N, 64), out,
                  epilogue=(_rand(31, N, lo=0.5, hi=1.5), None, _rand(32, 64)))
    return {"out": out}


def _epi_check(variant, o):
    _, s, d = graph(variant)
    exact, mass = _sum_ref(d, s, _rand(30, N, 64))
    scale = _rand(31, N, lo=0.5, hi=1.5).double()[:, None]
    _sum_close("out", o["out"], exact * scale + _rand(32, 64).double(), mass, scale)


def _generic_run(variant):
    g, _, _ = graph(variant)
    x = _rand(40, N, 3).requires_grad_()
    y = _rand(41, N, 3)
    g.ndata["x"], g.ndata["y"] = x, y
    g.update_all(fn.u_mul_v("x", "y", "m"), fn.max("m", "h"))  # k_lb_fixup
    hmax = g.ndata["h"].detach()
    g.update_all(fn.u_mul_v("x", "y", "m"), fn.sum("m", "s"))
    (gx,) = th.autograd.grad(g.ndata["s"], x, _rand(42, N, 3))  # k_lb_fixup<BWD>
    return {"max": hmax, "grad_lhs": gx}


def _generic_check(variant, o):
    _, s, d = graph(variant)
    x, y, go = _rand(40, N, 3), _rand(41, N, 3), _rand(42, N, 3)
    ref = th.full((N, 3), float("-inf"), device=DEV).index_reduce_(0, d, x[s] * y[d], "amax")
    has = th.bincount(d, minlength=N) > 0
    assert th.equal(o["max"][has], ref[has])
    # d sum / dx[u] = the sum over u's out-edges of y[v] * grad_out[v]
    _sum_close("grad_lhs", o["grad_lhs"], *_sum_ref(s, d, y * go))


def _run_gat(slopes):
    H, D = 4, 4
    # slopes "1": the forward keeps the slope aggregates (k_gat_fwd_fixup<LS>) and the backward
    # is the source-side walk (k_gat_bwd_fixup with_vec = 1); "0": the plain forward and the
    # destination-side walk too (with_vec = 0)
    env = {"DGLMI_GAT_SLOPES": slopes, "DGLMI_GAT_EDGE_POS": "0"}

    def inputs():
        return [_rand(50, N, H, D), _rand(51, N, H, 1), _rand(52, N, H, 1), _rand(53, N, H, D)]

    def run(variant):
        g, _, _ = graph(variant)
        ft, el, er, go = inputs()
        with _env(**env):
            leaves = [t.requires_grad_() for t in (ft, el, er)]
            out = B.fused_gat(g, *leaves, 0.2)
            gf = th.autograd.grad(out, leaves, go)
        return {"out": out.detach(), "g_ft": gf[0], "g_el": gf[1], "g_er": gf[2]}

    def check(variant, o):
        from test_fused_gat_gpu import dense_gat
        src, dst = hub_edges(variant)
        ft, el, er, go = inputs()
        fd, eld, erd = (t.double().requires_grad_() for t in (ft, el, er))
        ref = dense_gat(src, dst, N, fd, eld, erd, 0.2)
        gr = th.autograd.grad(ref, (fd, eld, erd), go.double())
        assert th.allclose(o["out"].double(), ref, rtol=1e-4, atol=1e-4)
        for name, b in zip(("g_ft", "g_el", "g_er"), gr):
            assert th.allclose(o[name].double(), b, rtol=1e-3, atol=1e-3), name
    return run, check


def _run_softmax(H):
    def run(variant):
        from dgl.nn.pytorch import edge_softmax
        g, s, _ = graph(variant)
        e = (4 * _rand(60 + H, len(s), H, 1)).requires_grad_()
        a = edge_softmax(g, e)
        (ge,) = th.autograd.grad(a, e, _rand(80 + H, len(s), H, 1))
        return {"out": a.detach(), "grad": ge}

    def check(variant, o):
        _, s, d = graph(variant)
        e, go = (4 * _rand(60 + H, len(s), H, 1)).double(), _rand(80 + H, len(s), H, 1).double()
        mx = th.full((N, H, 1), -1e300, dtype=th.float64, device=DEV).index_reduce_(0, d, e, "amax")
        ex = th.exp(e - mx[d])
        ref = ex / th.zeros(N, H, 1, dtype=th.float64, device=DEV).index_add_(0, d, ex)[d]
        dot = th.zeros(N, H, 1, dtype=th.float64, device=DEV).index_add_(0, d, ref * go)
        assert th.allclose(o["out"].double(), ref, rtol=1e-4, atol=1e-9)
        assert th.allclose(o["grad"].double(), ref * (go - dot[d]), rtol=1e-3, atol=1e-8)
    return run, check


def _plan_run(variant):
    src, dst = hub_edges(variant)
    with open_hub_gates():
        g = device_block_gidx(N, N, th.from_numpy(src).to(DEV).int(), th.from_numpy(dst).to(DEV).int())
        out, gx = th.empty(N, 64, device=DEV), th.empty(N, 64, device=DEV)
        x = _rand(70, N, 64)
        K.copy_reduce("sum", g, 0, x, out)
        K.backward_copy_reduce("sum", g, 0, x, out, _rand(71, N, 64), gx)
        assert g._hub_plans["in"] is not None and g._hub_plans["out"] is not None
        virt = g._hub_plans["in" if variant != "swapped" else "out"]
        ptr = virt._keep[3][:8 * virt.num_hubs + 1]
        assert int((ptr[1:] - ptr[:-1]).max()) > 33 * 8  # a virtual row of more than kFixSeg chunks
    return {"out": out, "grad_src": gx}


def _plan_check(variant, o):
    _, s, d = graph(variant)
    _sum_close("out", o["out"], *_sum_ref(d, s, _rand(70, N, 64)))
    _sum_close("grad_src", o["grad_src"], *_sum_ref(s, d, _rand(71, N, 64)))


CASES = {
    "sum_f64": _run_sum(64),    # k_chunk_fixup, float4 slots (and the source gradient)
    "sum_f18": _run_sum(18),    # float2 slots
    "sum_f17": _run_sum(17),    # single-float slots
    "sum_f6": _run_sum(6),      # k_lane_fixup
    "max_f64": _run_maxmin("max"),
    "min_f64": _run_maxmin("min"),
    "sum_epilogue": (_epi_run, _epi_check),       # k_chunk_fixup<EPI>
    "generic": (_generic_run, _generic_check),    # k_lb_fixup, forward and BWD
    "gat_slopes": _run_gat("1"),
    "gat_dst_walk": _run_gat("0"),
    "softmax_h1": _run_softmax(1),                # k_sm_fixup, K = 64
    "softmax_h8": _run_softmax(8),                # K = 32
    "planned_sum": (_plan_run, _plan_check),      # k_chunk_fixup<PLAN>
}


def run_case(name, variant):
    out = CASES[name][0](variant)
    th.cuda.synchronize()
    return out


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(CASES))
def test_fixup_case(name, variant):
    first = run_case(name, variant)
    again = run_case(name, variant)
    for k in first:
        assert th.equal(first[k], again[k]), k  # deterministic
    CASES[name][1](variant, first)


def test_hub_rows_start_where_the_docstring_says():
    """The in-CSR the library builds has the hub rows on (aligned) or five past (shifted)
    multiples of 64, with the degrees of HUB_DEGREES."""
    for variant, off in (("aligned", 0), ("shifted", 5)):
        g, _, _ = graph(variant)
        ptr = g._graph.get_immutable_gidx(DEV).in_csr.indptr.cpu().numpy().astype(np.int64)
        hubs = 2 * np.arange(len(HUB_DEGREES)) + 1
        assert (ptr[hubs] % 64 == off).all()
        assert (ptr[hubs + 1] - ptr[hubs] == np.array(HUB_DEGREES)).all()
