"""tests/generic_ref.py against the C oracle (oracle.binary_reduce) on the 20-node graph:
the numpy restatement is checked here, without a GPU, before tests/test_generic_shapes_gpu.py
compares any kernel with it.

Every (lhs, op, rhs, reducer) of tests/golden/make_golden.CASES, with the broadcast operand
none, the lhs or the rhs (features of graphs.binary_case_features) and a random grad_out.
Bounds: the oracle's own 1e-4 (rtol = atol) for sums and gradients, equality for max / min
and for reducer "none".  Gradients are compared in the kernel's full shape (oracle
backward_raw) and in the operand's shape (after reduce_grad); maps are checked on one case.
"""
import numpy as np
import pytest

import generic_ref as R
from graphs import CODE, binary_case_features, g20
from make_golden import CASES
from oracle import oracle as O


def _ends(src, dst, t):
    return {"u": src, "v": dst, "e": np.arange(len(src))}[t]


def _ref_case(red, op, src, dst, n, lt, rt, lv, rv, go, lmap=None, rmap=None, omap=None,
              out_rows=None):
    """out, full-shape (grad_lhs, grad_rhs) and their operand-shape sums, all fp64 (max / min /
    none forward: fp32), through the maps when given (go is indexed like the mapped output)."""
    L = R.through(lv, _ends(src, dst, lt), lmap)
    Rr = L if op == "use_lhs" else R.through(rv, _ends(src, dst, rt), rmap)
    t = R.EdgeTerms(op, L, Rr)
    base = "sum" if red == "mean" else red
    orow = np.arange(n) if omap is None else omap
    if base == "none":
        out, go_e, out_e = t.e32, go, None
    else:
        out, _ = R.reduce_forward(base, t, dst, n)
        scale = 1.0
        if red == "mean":
            scale = 1.0 / np.maximum(np.bincount(dst, minlength=n), 1).reshape((n,) + (1,) * len(t.out))
            out = out * scale
        go_e = (go[orow] * scale)[dst]
        out_e = out[dst]
    gl, _, gr, _ = R.edge_grads(base, t, go_e, out_e)
    grads = []
    for tgt, g, table, mp in ((lt, gl, lv, lmap), (rt, gr, rv, rmap)):
        if tgt is None:
            grads.append(None)
            continue
        rows = table.shape[0]
        if tgt == "e":
            full = R.place(rows, g, mp, 0.0)
        else:
            k = n if mp is None else rows
            ends = _ends(src, dst, tgt)
            full, _ = R.scatter_sum(g, np.abs(g), ends if mp is None else mp[ends], k)
        grads.append((full, R.reduce_to(full, table.shape[1:])[0]))
    if base != "none":
        out = R.place(out_rows or n, out, omap, R.IDENTITY[base] if red != "mean" else 0.0)
    return out, grads


def _variants():
    seen = set()
    for lhs, op, rhs, red, bc in CASES:
        for b in ("none", "lhs", "rhs", bc):
            b = {"lhs": lhs, "rhs": rhs}.get(b, b)
            if op == "use_lhs" or b is None:
                b = "none"
            key = (lhs, op, rhs, red, b)
            if key not in seen:
                seen.add(key)
                yield key


@pytest.mark.parametrize("lhs,op,rhs,red,bc", list(_variants()),
                         ids=lambda v: "-" if v is None else str(v))
def test_reference_matches_oracle(lhs, op, rhs, red, bc):
    src, dst, n = g20()
    m = len(src)
    g = O.RefGraph(src, dst, n)
    d = binary_case_features(n, m, lhs, rhs or "u", "mul" if op == "use_lhs" else op, bc)
    lv = d[lhs]
    rv = d[rhs] if rhs else None
    out_rows = m if red == "none" else n
    rs = np.random.RandomState(5)
    if op == "use_lhs":
        o_out = O.copy_reduce(red, g, CODE[lhs], lv, out_rows)
        go = rs.uniform(-1, 1, o_out.shape).astype(np.float32)
        _, o_gl = O.copy_reduce(red, g, CODE[lhs], lv, out_rows, grad_out=go)
        o_gr = None
    else:
        o_out = O.binary_reduce(red, op, g, CODE[lhs], CODE[rhs], lv, rv, out_rows)
        go = rs.uniform(-1, 1, o_out.shape).astype(np.float32)
        _, o_gl, o_gr = O.binary_reduce(red, op, g, CODE[lhs], CODE[rhs], lv, rv, out_rows,
                                        grad_out=go)
    out, grads = _ref_case(red, op, src, dst, n, lhs, rhs, lv, rv, go)
    assert out.shape == o_out.shape
    if red in ("max", "min", "none"):
        assert out.dtype == np.float32
        np.testing.assert_array_equal(out, o_out)
    else:
        np.testing.assert_allclose(out, o_out, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(grads[0][1], o_gl, rtol=1e-4, atol=1e-4)
    if rhs:
        np.testing.assert_allclose(grads[1][1], o_gr, rtol=1e-4, atol=1e-4)
        # the kernel's shape: the oracle's un-reduced gradients
        if red != "mean":
            for want in (0, 1):
                raw = O.backward_raw(red, op, g, CODE[lhs], CODE[rhs], lv, rv, o_out, go, want)
                assert raw.shape == grads[want][0].shape
                np.testing.assert_allclose(grads[want][0], raw, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("red", ["sum", "max"])
@pytest.mark.parametrize("lhs,op,rhs,lshape,rshape", [
    ("u", "sub", "v", (3, 1), (3, 4)),
    ("e", "dot", "v", (2, 1, 3), (1, 4, 3)),
    ("v", "div", "u", (5,), (5,)),
])
def test_reference_maps_match_oracle(lhs, op, rhs, lshape, rshape, red):
    """Injective, non-identity lhs / rhs / out maps into tables of twice the rows: reads go
    through the maps, unaddressed output rows keep the identity and unaddressed gradient
    rows are 0, as in the oracle."""
    src, dst, n = g20()
    m = len(src)
    g = O.RefGraph(src, dst, n)
    rs = np.random.RandomState(9)
    rows = {"u": n, "v": n, "e": m}
    lmap = rs.permutation(2 * rows[lhs])[:rows[lhs]]
    rmap = rs.permutation(2 * rows[rhs])[:rows[rhs]]
    omap = rs.permutation(2 * n)[:n]
    lv = rs.uniform(-1, 1, (2 * rows[lhs],) + lshape).astype(np.float32)
    rv = (rs.uniform(0.5, 1.5, (2 * rows[rhs],) + rshape) * rs.choice([-1, 1], (2 * rows[rhs],) + rshape)).astype(np.float32)
    # the oracle indexes an edge map by CSR position (out-CSR forward, in-CSR backward);
    # generic_ref and the engine index it by edge id
    def by_pos(mp, tgt, csr):
        return mp[csr[2]] if tgt == "e" else mp
    o_out = O.binary_op_reduce_raw(red, op, g, CODE[lhs], CODE[rhs], lv, rv, 2 * n,
                                   by_pos(lmap, lhs, g.out_csr), by_pos(rmap, rhs, g.out_csr), omap)
    go = rs.uniform(-1, 1, o_out.shape).astype(np.float32)
    out, grads = _ref_case(red, op, src, dst, n, lhs, rhs, lv, rv, go, lmap, rmap, omap, 2 * n)
    if red == "max":
        np.testing.assert_array_equal(out, o_out)
    else:
        np.testing.assert_allclose(out, o_out, rtol=1e-4, atol=1e-4)
    untouched = np.setdiff1d(np.arange(2 * n), omap)
    assert (out[untouched] == R.IDENTITY[red]).all()
    for want, mp, table in ((0, lmap, lv), (1, rmap, rv)):
        raw = O.backward_raw(red, op, g, CODE[lhs], CODE[rhs], lv, rv, o_out, go, want,
                             by_pos(lmap, lhs, g.in_csr), by_pos(rmap, rhs, g.in_csr), omap)
        np.testing.assert_allclose(grads[want][0], raw, rtol=1e-4, atol=1e-4)
        assert (grads[want][0][np.setdiff1d(np.arange(table.shape[0]), mp)] == 0).all()


def test_assert_within_rejects_nan_and_excess():
    """The bound check of the GPU tests: a NaN element or row (what a skipped store leaves in
    a NaN-filled buffer) fails, as does an infinity, an element outside its bound, and a NaN
    in the reference or the bound."""
    exact = np.arange(12, dtype=np.float64).reshape(3, 4)
    bound = np.full((3, 4), 1e-3)
    R.assert_within(exact.astype(np.float32), exact, bound, "ok")
    for spoil in (lambda a: a.__setitem__((1, 2), np.nan), lambda a: a.__setitem__(2, np.nan),
                  lambda a: a.__setitem__((0, 0), np.inf), lambda a: a.__setitem__((0, 3), 3.01)):
        got = exact.astype(np.float32)
        spoil(got)
        with pytest.raises(AssertionError):
            R.assert_within(got, exact, bound, "spoilt")
    for arr in (exact, bound):
        hurt = arr.copy()
        hurt[1, 1] = np.nan
        with pytest.raises(AssertionError):
            R.assert_within(exact.astype(np.float32), *((hurt, bound) if arr is exact else (exact, hurt)), "nan ref")


def test_feature_shapes_and_reduce_to():
    assert R.feature_shapes("mul", (8, 32), (32,)) == ((8, 32), (1, 32), (8, 32), (8, 32), 1)
    assert R.feature_shapes("dot", (4, 1, 8), (1, 5, 8)) == ((4, 1, 8), (1, 5, 8), (4, 5, 8), (4, 5), 8)
    a = np.arange(2 * 4 * 5 * 8, dtype=np.float64).reshape(2, 4, 5, 8)
    r, k = R.reduce_to(a, (4, 1, 8))
    assert k == 5 and np.array_equal(r, a.sum(2, keepdims=True))
    r, k = R.reduce_to(a, (8,))
    assert k == 20 and r.shape == (2, 8) and np.array_equal(r, a.sum((1, 2)))
    assert R.reduce_to(a, (4, 5, 8))[1] == 1


# every dot shape of the per-edge kernels' table (tests/test_sddmm_shapes_gpu.py) that the
# group kernel's order applies to: len % 4 == 0 and len / 4 a power of two
GROUP_DOTS = [(1, 4), (2, 4), (1, 8), (3, 4), (1, 16), (5, 4), (4, 8), (9, 4), (2, 32), (17, 4),
              (1, 128), (33, 4), (1, 256), (65, 4), (2, 256), (1, 512), (129, 4), (3, 256),
              (2, 512), (1, 1024)]


def _dot_operands(shape, rows=1501):
    rs = np.random.RandomState(shape[0] * 4099 + shape[1])
    return (rs.uniform(-1, 1, (rows,) + shape).astype(np.float32),
            rs.uniform(-1, 1, (rows,) + shape).astype(np.float32))


@pytest.mark.parametrize("shape", GROUP_DOTS, ids=lambda s: "%dx%d" % s)
def test_dot_group32(shape):
    """The group kernel's summation order: within (len + 1) 2^-24 majorant of fp64 (len
    products and len - 1 additions in any order, the additions of partial sums no larger than
    the majorant; one more for the fold from 0), the sequential chain itself at len = 4, and
    a different rounding from the chain in more than a quarter of the elements from len = 32
    -- so that nobody "simplifies" it to the sequential order."""
    L, Rr = _dot_operands(shape)
    t = R.EdgeTerms("dot", L, Rr)
    got = R.dot_group32(L, Rr)
    assert got.shape == t.e32.shape and got.dtype == np.float32
    R.assert_within(got, t.e64, (shape[1] + 1) * R.EPS * t.emaj, "dot_group32 %s" % (shape,))
    if shape[1] == 4:
        assert np.array_equal(got, t.e32)
    if shape[1] >= 32:
        assert (got != t.e32).mean() > 0.25, (got != t.e32).mean()


@pytest.mark.parametrize("op", ["add", "sub", "mul", "div", "dot", "use_lhs"])
def test_edge_grads32_within_bound_of_fp64(op):
    """The fp32 restatement of the per-edge gradients against edge_grads' fp64 values, at
    the bound the GPU tests use for per-edge gradients without a dot chain."""
    rs = np.random.RandomState(17)
    shape = (5, 8) if op == "dot" else (40,)
    L = rs.uniform(-1, 1, (997,) + shape).astype(np.float32)
    Rr = rs.uniform(-1, 1, (997,) + shape)
    if op == "div":
        Rr = (np.abs(Rr) + 0.5) * np.where(Rr < 0, -1.0, 1.0)
    Rr = Rr.astype(np.float32)
    t = R.EdgeTerms(op, L, L if op == "use_lhs" else Rr)
    go = rs.uniform(-1, 1, (997,) + t.out).astype(np.float32)
    gl, glmaj, gr, grmaj = R.edge_grads("none", t, go)
    gl32, gr32 = R.edge_grads32(op, L, Rr, go)
    assert gl32.shape == gl.shape
    R.assert_within(gl32, gl, R.edge_bound(glmaj, 0), op + " grad lhs")
    if op == "use_lhs":
        assert gr32 is None and np.array_equal(gl32, go)
    else:
        R.assert_within(gr32, gr, R.edge_bound(grmaj, 0), op + " grad rhs")
    if op in ("add", "sub"):
        assert np.array_equal(gl32, go) and np.array_equal(gr32, go if op == "add" else -go)
