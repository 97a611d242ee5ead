"""The generic reduce kernels (csrc/kernels_generic.hip) at wide rows, with broadcasts and
with operand maps, on graphs with hub rows (needs an MI355X).

Reference: tests/generic_ref.py (numpy; checked against the C oracle on the CPU by
tests/test_generic_ref_cpu.py).  grad_out is always random, never ones, so a wrong index in
a grad_out / fwd_out read changes the result.

Graphs: ``powerlaw(2000, 30000, seed=7)`` ("in": the in-CSR walks -- forward reductions and
the gradients of v operands -- see the hubs) and the same with source and destination
exchanged ("swap": the out-CSR walks, the gradients of u operands, see them).  Maximum
degree 5741, 15 rows over 264 entries, 317 over 8, 539 empty, duplicate edges (exact ties at
a maximum).  fast_chunk_edges gives K = 8 positions per chunk at this size for every width, so
a row over 8 entries is cut and one over 264 has more than one fixup segment (kFixSeg = 32).

Which kernel a case reaches, by the rules at the time of writing (lane_bits_for,
generic_lb_supported, sddmm_supported, the fast-path gates of capi.cpp forward / backward).
D = floats of an output row, Dg = D * len = floats of a gradient row, slots = ceil(row / 64):

    forward, reducer sum / max / min / prod       D <= 256   k_lb_reduce<BWD=false> + k_lb_fixup
                                                  D >  256   k_node_fwd
    forward, reducer none (broadcast pairs only)             k_edge_fwd<BC=true>
    gradient of a node operand (u: out-CSR,       Dg <= 256  k_lb_reduce<BWD=true> + k_lb_fixup
      v: in-CSR)                                  Dg >  256  k_node_bwd
    gradient of an edge operand                              k_edge_bwd, except: reducer sum, no
      broadcast, no maps and Dg <= 8 (not 5, 7) or Dg % 4 == 0 (dot: len % 4 == 0 too) go to
      kernels_sddmm.hip -- here (1,), (2,), (200,), (256,), dot (16,12) and dot (40,8)

    shape                      D     Dg    forward slots        gradient slots
    (1,) (2,) (5,)             1 2 5       1 (groups of 1 2 8 lanes, (5,) partly used)
    (65,)                      65          2 (one lane in the last)
    (130,)                     130         3
    (200,)                     200         4, partial
    (256,)                     256         4, full
    (257,)                     257         row-per-group        row-per-group
    dot (3,5)                  3     15    1                    1
    dot (16,12)                16    192   1                    3
    dot (70,3)                 70    210   2                    4
    dot (40,8)                 40    320   1                    row-per-group
    (5,3,4) x (3,1)            60          1, BC
    (4,1,6) x (1,5,6)          120         2, BC (both sides broadcast)
    (8,32) x (32,)             256         4, BC (ranks differ)
    (3,1) x (3,30)             90          2, BC
    dot (4,1,8) x (1,5,8)      20    160   1, BC                3, BC
    dot (9,1,4) x (9,8,4)      72    288   2, BC                row-per-group, BC

u_mul_e with reducer sum (and its (N,H,D) x (E,H,1) / (N,D) x (E,1) broadcasts) goes to
kernels_spmm.hip and is kept out of the rotation.  Maps (test_maps) switch every specialised
path off: forward k_lb_reduce through out_map after an identity fill, gradients
k_lb_reduce<BWD> / k_edge_bwd through the operand's map after a zero fill.  If those rules
change, revisit this table and ``_coverage``.

Bounds (generic_ref.node_sum_bound / edge_bound):

* empty rows: exactly the identity; max / min forward and reducer none: bit-equal to the fp32
  restatement; the max / min tie mask comes from that restatement;
* node-owned sums, forward and gradients: 1e-4 + (512 + deg/128 + len + 2) 2^-24 mass, the
  bound of test_generic_gpu._check_node_sum with the dot length added to the chain;
* per-edge gradients: (len + 6) 2^-24 majorant -- six roundings around a len-term dot.  In
  the operand's shape (autograd sums the kernel's rows over the k broadcast positions in fp32)
  k - 1 more: an fp32 sum of k terms in any order is within (k - 1) 2^-24 of their mass;
* prod forward: (4 deg + 4) 2^-24 |exact| (deg factors with one rounding each, deg multiplies,
  doubled); prod gradient of an edge operand: (4 deg + 12) 2^-24 |exact|.  The node-owned prod
  gradient stays covered by the 20-node graph only (test_kernels_gpu).
* every case run twice is bit-equal;
* every bound check requires finite values first and counts anything not <= its bound as
  outside: the direct calls start from NaN-filled buffers, so a skipped store fails.
"""
import zlib

import numpy as np
import pytest
import torch as th

import dgl
import generic_ref as R
from dgl import kernel as K
from graphs import CODE, powerlaw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

OPS4 = ("add", "sub", "mul", "div")
PAIRS = (("u", "v"), ("e", "v"), ("u", "e"), ("v", "u"))
PLAIN = [(1,), (2,), (5,), (65,), (130,), (200,), (256,), (257,)]
DOTS = [(3, 5), (16, 12), (70, 3), (40, 8)]
BCAST = [((5, 3, 4), (3, 1)), ((4, 1, 6), (1, 5, 6)), ((8, 32), (32,)), ((3, 1), (3, 30))]
BCAST_DOT = [((4, 1, 8), (1, 5, 8)), ((9, 1, 4), (9, 8, 4))]
# min on one shape per slot count (1, 2, 3, 4, row-per-group), plain, dot and broadcast
MIN_SHAPES = {((5,), (5,)), ((65,), (65,)), ((130,), (130,)), ((200,), (200,)), ((257,), (257,)),
              ((16, 12), (16, 12)), ((40, 8), (40, 8)), ((4, 1, 6), (1, 5, 6)),
              ((9, 1, 4), (9, 8, 4))}


def _slots(row):
    return 5 if row > 256 else -(-row // 64)  # 5: row-per-group


def _is_dot(ls, rs):
    return (ls, rs) in [(s, s) for s in DOTS] or (ls, rs) in BCAST_DOT or (rs, ls) in BCAST_DOT


def _cases():
    shapes = [(s, s) for s in PLAIN + DOTS]
    for a, b in BCAST + BCAST_DOT:
        shapes += [(a, b), (b, a)]
    cases = []
    for i, (ls, rs) in enumerate(shapes):
        reds = ["sum", "max"] + (["min"] if (ls, rs) in MIN_SHAPES else []) + (["none"] if ls != rs else [])
        for gi, gk in enumerate(("in", "swap")):
            for ri, red in enumerate(reds):
                op = "dot" if _is_dot(ls, rs) else OPS4[(i + 2 * gi + ri) % 4]
                pair = PAIRS[(i // 2 + gi + 3 * ri) % 4]
                if op == "mul" and red == "sum" and pair == ("u", "e"):
                    pair = ("e", "v")  # u_mul_e_sum is the specialised SpMM's
                cases.append((gk, red, op) + pair + (ls, rs))
    return cases


def _coverage(cases):
    """The rotation keeps what the module docstring promises.  A slot count is taken from the
    forward row (D) and from the gradient row (Dg) alike: an op "meets" a count that either
    direction reaches (dot reaches row-per-group only in the backward: no dot shape has
    D > 256)."""
    by_slot, by_bc, hub_node, edge_rpg, min_slots = set(), set(), set(), set(), set()
    for gk, red, op, lhs, rhs, ls, rs in cases:
        _, _, full, out, ln = R.feature_shapes(op, ls, rs)
        D, Dg = int(np.prod(out)), int(np.prod(full))
        assert not (op == "mul" and red == "sum" and {lhs, rhs} == {"u", "e"})
        for s in {_slots(D), _slots(Dg)}:
            by_slot.add((op, s))
            if red == "min":
                min_slots.add(s)
        by_bc.add(((lhs, rhs), ls != rs))
        if Dg > 256:
            # a node operand whose walk sees the hubs, and an edge operand
            if (gk == "in" and "v" in (lhs, rhs)) or (gk == "swap" and "u" in (lhs, rhs)):
                hub_node.add((ls, rs))
            if "e" in (lhs, rhs):
                edge_rpg.add((ls, rs))
    assert by_slot >= {(op, s) for op in OPS4 + ("dot",) for s in (1, 2, 3, 4, 5)}, by_slot
    assert by_bc == {(p, b) for p in PAIRS for b in (False, True)}
    assert min_slots == {1, 2, 3, 4, 5}
    wide = {((257,), (257,)), ((40, 8), (40, 8)), ((9, 1, 4), (9, 8, 4)), ((9, 8, 4), (9, 1, 4))}
    assert hub_node == wide and edge_rpg == wide, (hub_node, edge_rpg)
    for shape in {c[5:] for c in cases}:
        for gk in ("in", "swap"):
            assert {"sum", "max"} <= {c[1] for c in cases if c[5:] == shape and c[0] == gk}


CASES = _cases()
_coverage(CASES)


def _case_id(c):
    gk, red, op, lhs, rhs, ls, rs = c
    sh = "x".join(map(str, ls)) + ("" if ls == rs else "_" + "x".join(map(str, rs)))
    return "%s-%s-%s_%s_%s-%s" % (gk, red, lhs, op, rhs, sh)


_GRAPHS = {}


def graph(kind):
    if kind not in _GRAPHS:
        src, dst, n = powerlaw(2000, 30000, seed=7)
        if kind == "swap":
            src, dst = dst, src
        hub = np.bincount(dst if kind == "in" else src, minlength=n)
        # what the table above relies on
        assert hub.max() == 5741 and (hub > 264).sum() == 15 and (hub > 8).sum() == 317
        assert (hub == 0).sum() == 539
        g = dgl.DGLGraph()
        g.add_nodes(n)
        g.add_edges(src, dst)
        _GRAPHS[kind] = (src, dst, n, g, g._graph.get_immutable_gidx(DEV))
    return _GRAPHS[kind][:3] + _GRAPHS[kind][4:]


def _ends(src, dst, t):
    return {"u": src, "v": dst, "e": np.arange(len(src))}[t]


def _seed(*key):
    return zlib.crc32(repr(key).encode()) % (2 ** 31)


def _feats(rs, rows, shape, away_from_zero=False, near_one=False):
    x = rs.uniform(-1, 1, (rows,) + shape)
    sign = np.where(x < 0, -1.0, 1.0)
    if near_one:       # prod: magnitude in [0.99, 1.01]
        x = (0.99 + 0.02 * np.abs(x)) * sign
    elif away_from_zero:  # a divisor: magnitude in [0.5, 1.5]
        x = (np.abs(x) + 0.5) * sign
    return x.astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _assert_within(got, exact, bound, tag):
    got = got.astype(np.float64).reshape(exact.shape)
    assert np.isfinite(got).all(), "%s: %d of %d not finite (left unwritten?)" % (
        tag, int((~np.isfinite(got)).sum()), got.size)
    err = np.abs(got - exact)
    bad = ~(err <= bound)  # a NaN anywhere counts as outside
    assert not bad.any(), "%s: %d of %d outside, max excess %g (err %g)" % (
        tag, int(bad.sum()), bad.size, float((err - bound).max()), float(err.max()))


def _expected(gk, red, op, lhs, rhs, lv, rv, go, maps=(None, None, None)):
    """The forward output and both gradients in the kernel's (full) shape.

    Returns (fwd, grads).  fwd: ("bits", out32) or ("sum", exact, bound, empty_rows), with
    rows as the kernel writes them (through out_map).  grads[w]: dict(owner, exact, maj, deg,
    zero): exact and majorant / mass per row of the operand's table, deg (node-owned: terms
    per row; None for an edge operand) and the rows that must be exactly 0."""
    src, dst, n, _ = graph(gk)
    lmap, rmap, omap = maps
    L = R.through(lv, _ends(src, dst, lhs), lmap)
    Rr = R.through(rv, _ends(src, dst, rhs), rmap)
    t = R.EdgeTerms(op, L, Rr)
    orow = np.arange(n) if omap is None else omap
    deg_in = np.bincount(dst, minlength=n)
    cols = (1,) * len(t.out)
    if red == "none":
        fwd, go_e, out_e = ("bits", t.e32), go, None
    else:
        go_e = go[orow][dst]
        rows_total = go.shape[0]
        if red == "sum":
            exact, mass = R.reduce_forward(red, t, dst, n)
            bound = R.node_sum_bound(mass, deg_in.reshape((n,) + cols), t.len)
            empty = np.ones(rows_total, bool)
            empty[orow[deg_in > 0]] = False
            fwd = ("sum", R.place(rows_total, exact, omap, 0.0), R.place(rows_total, bound, omap, 0.0), empty)
            out_e = None
        else:
            out32, _ = R.reduce_forward(red, t, dst, n)
            fwd = ("bits", R.place(rows_total, out32, omap, R.IDENTITY[red]))
            out_e = out32[dst]
    gl, glmaj, gr, grmaj = R.edge_grads(red, t, go_e, out_e)
    grads = []
    for tgt, g, gmaj, table, mp in ((lhs, gl, glmaj, lv, lmap), (rhs, gr, grmaj, rv, rmap)):
        rows = table.shape[0]
        zero = np.ones(rows, bool)
        if tgt == "e":
            exact, maj, deg = R.place(rows, g, mp, 0.0), R.place(rows, gmaj, mp, 0.0), None
            zero[np.arange(len(src)) if mp is None else mp] = False
        else:
            ends = _ends(src, dst, tgt)
            ends = ends if mp is None else mp[ends]
            exact, maj = R.scatter_sum(g, gmaj, ends, rows)
            deg = np.bincount(ends, minlength=rows)
            zero = deg == 0
        grads.append(dict(owner=tgt, exact=exact, maj=maj, deg=deg, zero=zero, len=t.len))
    return fwd, grads


def _check_fwd(fwd, got, tag):
    if fwd[0] == "bits":
        assert got.shape == fwd[1].shape, tag
        same = _bits(got) == _bits(fwd[1])
        assert same.all(), "%s: %d of %d not bit-equal" % (tag, int((~same).sum()), same.size)
    else:
        _, exact, bound, empty = fwd
        _assert_within(got, exact, bound, tag)
        assert (got[empty] == 0).all(), tag + ": empty rows"


def _check_grad(e, got, shape, tag):
    """got against e (see _expected), in the kernel's shape or summed to ``shape``."""
    exact, k = R.reduce_to(e["exact"], shape)
    maj, _ = R.reduce_to(e["maj"], shape)
    got = got.reshape(exact.shape)
    if e["deg"] is None:
        bound = R.edge_bound(maj, e["len"], k - 1)
    else:
        bound = R.node_sum_bound(maj, e["deg"].reshape((-1,) + (1,) * (exact.ndim - 1)), e["len"])
    _assert_within(got, exact, bound, tag)
    assert (got[e["zero"]] == 0).all(), tag + ": rows without terms"


def _inputs(case, near_one=False):
    gk, red, op, lhs, rhs, ls, rs = case
    src, dst, n, _ = graph(gk)
    rows = {"u": n, "v": n, "e": len(src)}
    rng = np.random.RandomState(_seed(case))
    lv = _feats(rng, rows[lhs], ls, near_one=near_one)
    rv = _feats(rng, rows[rhs], rs, away_from_zero=op == "div", near_one=near_one)
    out_shape = R.feature_shapes(op, ls, rs)[3]
    go = rng.uniform(-1, 1, (len(src) if red == "none" else n,) + out_shape).astype(np.float32)
    return lv, rv, go


def _autograd(case, lv, rv, go, need=(True, True)):
    gk, red, op, lhs, rhs, _, _ = case
    src, _, n, gidx = graph(gk)
    lt = th.from_numpy(lv).to(DEV).requires_grad_(need[0])
    rt = th.from_numpy(rv).to(DEV).requires_grad_(need[1])
    out = dgl.backend.binary_reduce(red, op, gidx, CODE[lhs], CODE[rhs], lt, rt,
                                    len(src) if red == "none" else n)
    out.backward(th.from_numpy(go).to(DEV).reshape(out.shape))
    return [out.detach().cpu().numpy()] + [None if x.grad is None else x.grad.cpu().numpy()
                                           for x in (lt, rt)]


def _same(a, b):
    return all((x is None and y is None) or np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def test_case_count():
    print("\ntest_generic_shapes_gpu: %d rotation cases, %d on broadcast pairs"
          % (len(CASES), sum(c[5] != c[6] for c in CASES)))
    assert len({_case_id(c) for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_shapes(case):
    """Forward and both gradients in the operands' shapes, through autograd."""
    gk, red, op, lhs, rhs, ls, rs = case
    lv, rv, go = _inputs(case)
    got = _autograd(case, lv, rv, go)
    fwd, grads = _expected(gk, red, op, lhs, rhs, lv, rv, go)
    tag = _case_id(case)
    _check_fwd(fwd, got[0], tag + " forward")
    _check_grad(grads[0], got[1], ls, tag + " grad lhs")
    _check_grad(grads[1], got[2], rs, tag + " grad rhs")
    assert _same(got, _autograd(case, lv, rv, go)), tag + ": two runs differ"


def _direct(case, lv, rv, go, out_rows, maps=(None, None, None)):
    """The C entries themselves: out, grad_lhs and grad_rhs in the kernel's shape.  Buffers
    start as NaN, so every element the kernels leave alone shows."""
    gk, red, op, lhs, rhs, ls, rs = case
    _, _, _, gidx = graph(gk)
    _, _, full, oshape, _ = R.feature_shapes(op, ls, rs)
    dev = [None if m is None else th.from_numpy(m.astype(np.int32)).to(DEV) for m in maps]
    lt, rt = th.from_numpy(lv).to(DEV), th.from_numpy(rv).to(DEV)
    nan = float("nan")
    out = th.full((out_rows,) + oshape, nan, device=DEV)
    K.binary_op_reduce(red, op, gidx, CODE[lhs], CODE[rhs], lt, rt, out, *dev)
    got = th.from_numpy(go).to(DEV)
    gl = th.full((lv.shape[0],) + full, nan, device=DEV)
    gr = th.full((rv.shape[0],) + full, nan, device=DEV)
    K.backward_lhs_binary_op_reduce(red, op, gidx, CODE[lhs], CODE[rhs], lt, rt, out, got, gl, *dev)
    K.backward_rhs_binary_op_reduce(red, op, gidx, CODE[lhs], CODE[rhs], lt, rt, out, got, gr, *dev)
    return [x.cpu().numpy() for x in (out, gl, gr)]


FULL_CASES = [(gk, ("sum", "max", "none")[(i + gi) % 3], "dot" if (a, b) in BCAST_DOT else OPS4[(i + gi) % 4])
              + PAIRS[(i + 2 * gi) % 4] + (a, b)
              for i, (a, b) in enumerate(BCAST + BCAST_DOT) for gi, gk in enumerate(("in", "swap"))]


@pytest.mark.parametrize("case", FULL_CASES, ids=_case_id)
def test_broadcast_gradients_in_kernel_shape(case):
    """The gradients as the kernels write them: the full broadcast shape times len, before
    _reduce_grad sums them."""
    gk, red, op, lhs, rhs, ls, rs = case
    lv, rv, go = _inputs(case)
    full = R.feature_shapes(op, ls, rs)[2]
    got = _direct(case, lv, rv, go, go.shape[0])
    fwd, grads = _expected(gk, red, op, lhs, rhs, lv, rv, go)
    tag = _case_id(case)
    _check_fwd(fwd, got[0], tag + " forward")
    _check_grad(grads[0], got[1], full, tag + " grad lhs")
    _check_grad(grads[1], got[2], full, tag + " grad rhs")
    assert _same(got, _direct(case, lv, rv, go, go.shape[0])), tag + ": two runs differ"


MAP_CASES = [("in", red, op, lhs, rhs, ls, rs)
             for (op, lhs, rhs, ls, rs) in (("sub", "u", "v", (5,), (5,)),
                                            ("div", "e", "v", (130,), (130,)),
                                            ("add", "u", "e", (4, 1, 6), (1, 5, 6)),
                                            # add / mul with lhs target above rhs target: the
                                            # entry swaps the operands, lhs_map with rhs_map,
                                            # and which gradient is wanted (NeedSwitchOrder)
                                            ("mul", "v", "u", (5,), (5,)),
                                            ("add", "e", "v", (130,), (130,)))
             for red in ("sum", "max")]


@pytest.mark.parametrize("case", MAP_CASES, ids=_case_id)
def test_maps(case):
    """lhs_map, rhs_map and out_map, int32, injective and not the identity: both operand
    tables and the output have twice the rows and are addressed through a random injection;
    the backward gets the same maps.  Output rows no map addresses hold the identity,
    gradient rows no map addresses are exactly 0."""
    gk, red, op, lhs, rhs, ls, rs = case
    src, dst, n, _ = graph(gk)
    rows = {"u": n, "v": n, "e": len(src)}
    rng = np.random.RandomState(_seed("maps", case))
    maps = tuple(rng.permutation(2 * k)[:k] for k in (rows[lhs], rows[rhs], n))
    assert all((m != np.arange(len(m))).any() for m in maps)
    lv = _feats(rng, 2 * rows[lhs], ls)
    rv = _feats(rng, 2 * rows[rhs], rs, away_from_zero=op == "div")
    oshape, full = R.feature_shapes(op, ls, rs)[3], R.feature_shapes(op, ls, rs)[2]
    go = rng.uniform(-1, 1, (2 * n,) + oshape).astype(np.float32)
    got = _direct(case, lv, rv, go, 2 * n, maps)
    fwd, grads = _expected(gk, red, op, lhs, rhs, lv, rv, go, maps)
    tag = _case_id(case)
    _check_fwd(fwd, got[0], tag + " forward")
    untouched = np.setdiff1d(np.arange(2 * n), maps[2])
    assert (got[0][untouched] == R.IDENTITY[red]).all(), tag + ": rows out_map does not address"
    for w, name in ((0, " grad lhs"), (1, " grad rhs")):
        _check_grad(grads[w], got[1 + w], full, tag + name)
        free = np.setdiff1d(np.arange(got[1 + w].shape[0]), maps[w])
        assert (got[1 + w][free] == 0).all(), tag + name + ": rows the map does not address"
    assert _same(got, _direct(case, lv, rv, go, 2 * n, maps)), tag + ": two runs differ"


# the forward always walks the in-CSR and an edge gradient is per edge: the "in" graph only
PROD_CASES = [("in", "prod", op, lhs, rhs) + ((ls, rs) if lhs == "e" else (rs, ls))
              for lhs, rhs in (("e", "v"), ("u", "e"))
              for ls, rs in [((5,), (5,)), ((65,), (65,)), ((200,), (200,)), ((5, 3, 4), (3, 1))]
              for op in ("mul", "div")]


@pytest.mark.parametrize("case", PROD_CASES, ids=_case_id)
def test_prod(case):
    """prod over hub rows: factors of magnitude 0.99 .. 1.01 keep a 5741-term product in
    range.  The forward and the gradient of the edge operand (grad_out * out / e * d e); in
    the broadcast case the edge operand has the full shape, so its gradient is not summed."""
    gk, red, op, lhs, rhs, ls, rs = case
    src, dst, n, _ = graph(gk)
    lv, rv, go = _inputs(case, near_one=True)
    w = 0 if lhs == "e" else 1
    got = _autograd(case, lv, rv, go, need=(w == 0, w == 1))
    t = R.EdgeTerms(op, lv[_ends(src, dst, lhs)], rv[_ends(src, dst, rhs)])
    out64, _ = R.reduce_forward("prod", t, dst, n)
    deg = np.bincount(dst, minlength=n).reshape((n,) + (1,) * len(t.out))
    tag = _case_id(case)
    _assert_within(got[0], out64, (4 * deg + 4) * R.EPS * np.abs(out64), tag + " forward")
    assert (got[0][deg.reshape(-1) == 0] == 1).all(), tag + ": empty rows"
    g = R.edge_grads("prod", t, go[dst], out64[dst])[2 * w]
    assert g.shape[1:] == (ls, rs)[w], "the edge operand has the full shape"
    _assert_within(got[1 + w], g, (4 * deg[dst] + 12) * R.EPS * np.abs(g), tag + " edge grad")
    assert _same(got, _autograd(case, lv, rv, go, need=(w == 0, w == 1))), tag + ": two runs differ"
