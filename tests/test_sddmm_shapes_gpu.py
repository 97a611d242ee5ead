"""The per-edge (g-SDDMM) kernels of csrc/kernels_sddmm.hip at every instance, bit for bit
(needs an MI355X).

k_sddmm_lane and k_sddmm_group produce every ``apply_edges`` builtin (reducer "none") and every
edge-owned gradient of reducers none / sum.  The C entries are called directly
(dgl.kernel.binary_op_reduce, backward_{lhs,rhs}_binary_op_reduce, copy_reduce,
backward_copy_reduce) on NaN-filled buffers, so an element a kernel leaves alone shows.

Reference: tests/generic_ref.py (numpy; checked on the CPU by tests/test_generic_ref_cpu.py).
``EdgeTerms.e32`` states add / sub / mul / div (one IEEE operation per element) and the lane
kernel's sequential dot, ``dot_group32`` the group kernel's dot in its own order (float4
partials, xor butterfly, slot fold), ``edge_grads32`` the per-edge gradients.  The library is
built with -ffp-contract=off, so all of these hold to equality.

Main graph: ``powerlaw(500, 6001, seed=7)``: 6001 = 1 (mod 4) edges, so the last iteration of
the group kernel is a tail at U = 4 and at U = 2; duplicate edges and empty rows.  Every case
runs in both item orders (edge-id order from the COO, in-CSR positions with the output
scattered by edge id) and twice in each; the four results are bit-equal.

Which kernel a shape reaches, by the rules at the time of writing (sddmm_supported, run_op,
run_group; restated in ``_supported`` / ``_config`` and asserted at import by ``_coverage``):

    kernel        widths NF            dot shapes (D, len)
    lane          1 2 3 4 6 8          (1,2) (1,3) (2,2) (1,4) (2,3) (3,2) (1,6) (2,4) (4,2) (1,8)
    group (4,1)   12 16                (3,4) (1,16)
    group (8,1)   20 32                (5,4) (4,8)
    group (16,1)  36 64     [48]       (9,4) (2,32)                       [(2,24)]
    group (32,1)  68 128               (17,4) (1,128)
    group (64,1)  132 256   [192]      (33,4) (1,256)                     [(16,12)]
    group (64,2)  260 512              (65,4) (2,256) (1,512)
    group (64,4)  516 768 1024         (129,4) (3,256) (2,512) (1,1024)   [(1,768)]
    neither       5 7 15 10            (3,5)

A dot of length 1 goes as mul.  The shapes in brackets are the "backward only" row: len % 4 == 0
but len / 4 is no power of two, so the forward runs the generic k_edge_fwd (sequential dot) and
only the gradients run k_sddmm_group; 48 and 192 also run the elementwise ops.  The "neither"
row runs the generic kernels both ways: the gate is tested from both sides.

Every op runs on every width with the target pairs rotating over (u,v) (e,v) (v,u) (u,e) (e,u)
(v,e); lane shapes take two pairs each, and the "backward only" dot shapes rotate over the four
pairs with an edge operand (their gradients are all they run in these kernels).  add / mul
swap their operands in the entry when the lhs target is above the rhs target (v,u / e,v /
e,u), sub / div / dot keep them, so v_sub_u,
e_div_u, v_dot_u reach the kernels with the roles COL / ROW exchanged.  Cases with an edge
operand also run both gradients with reducers none (grad_out per edge) and sum (per
destination row); the edge operand's comes from the per-edge kernels, the node operand's from
the reduce kernels.  copy_u / copy_e (OP_USE_LHS) run at every supported width.

Assertions:

* forward add / sub / mul / div / copy and the lane dot: finite, then ``np.array_equal`` with the
  fp32 restatement (+-0 are not told apart);
* group dot forward: equal to ``dot_group32`` and within (len + 1) 2^-24 majorant of fp64 (len
  products, len - 1 additions, one fold from 0; the second check knows nothing of the order);
* edge-owned gradients from the per-edge kernels: equal to ``edge_grads32`` and within
  ``generic_ref.edge_bound(maj, 0)`` of fp64;
* generic routes (the "neither" row, the forward of the "backward only" row, unaligned
  operands): the bounds of test_generic_shapes_gpu -- reducer none bit-equal to the sequential
  fp32 restatement, per-edge gradients within ``edge_bound(maj, len)``;
* node-owned gradients: ``generic_ref.node_sum_bound``, rows without terms exactly 0.

Further cases at NF 6, 12, 260 and dot (2,512): operands 4 bytes off 16-byte alignment (the
entry's aligned16 gate), the 64-bit index layout in in-CSR order, partial ``apply_edges`` on a
parent-eid subgraph, graphs of 1, 2, 3 and 5 edges.  Three larger graphs cross the grid-stride
loops (16 384 blocks: 65 536 edges a sweep at (64,4), 262 144 at (64,1), 4 194 304 for the lane
kernels and (4,1)).
"""
import contextlib
import zlib

import numpy as np
import pytest
import torch as th

import dgl
import dgl.function as fn
import generic_ref as R
from dgl import kernel as K
from graphs import CODE, powerlaw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

OPS4 = ("add", "sub", "mul", "div")
OPS = OPS4 + ("dot", "use_lhs")
PAIRS = (("u", "v"), ("e", "v"), ("v", "u"), ("u", "e"), ("e", "u"), ("v", "e"))
GROUP_CFGS = ((4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4))
# (row name, widths, dot shapes)
TABLE = (
    ("lane", (1, 2, 3, 4, 6, 8),
     ((1, 2), (1, 3), (2, 2), (1, 4), (2, 3), (3, 2), (1, 6), (2, 4), (4, 2), (1, 8))),
    ("group", (12, 16), ((3, 4), (1, 16))),
    ("group", (20, 32), ((5, 4), (4, 8))),
    ("group", (36, 64), ((9, 4), (2, 32))),
    ("group", (68, 128), ((17, 4), (1, 128))),
    ("group", (132, 256), ((33, 4), (1, 256))),
    ("group", (260, 512), ((65, 4), (2, 256), (1, 512))),
    ("group", (516, 768, 1024), ((129, 4), (3, 256), (2, 512), (1, 1024))),
    ("bwd_only", (48, 192), ((2, 24), (16, 12), (1, 768))),
    ("neither", (5, 7, 15, 10), ((3, 5),)),
)


def _supported(op, bwd, D, ln):
    """sddmm_supported, restated."""
    NF = D * ln
    if NF <= 0:
        return False
    if NF <= 8:
        return NF not in (5, 7)
    if NF % 4 or NF > 1024:
        return False
    if op == "dot" and ln > 1:
        if ln % 4:
            return False
        if bwd:
            return True
        S = ln // 4
        if S & (S - 1):
            return False
        # the kernel's last clause, S > L and S % L != 0, cannot hold for powers of two
    return True


def _config(NF):
    """run_op / run_lane / run_group, restated: ("lane", NF) or ("group", (L, NV))."""
    if NF <= 8:
        return ("lane", NF)
    for L in (4, 8, 16, 32, 64):
        if NF // 4 <= L:
            return ("group", (L, 1))
    return ("group", (64, 2) if NF // 4 <= 128 else (64, 4))


def _dims(op, shape):
    """(D, len) of a case's feature shape: (NF,) elementwise, (D, len) dot."""
    return (shape[0], shape[1]) if op == "dot" else (shape[0], 1)


def _instance(op, shape, bwd):
    """The kernel instance (kernel, NF or (L, NV), op, direction) a call reaches, None when
    the entry's gate sends it to the generic kernels."""
    D, ln = _dims(op, shape)
    if not _supported(op, bwd, D, ln):
        return None
    if op == "dot" and ln == 1:
        op = "mul"
    return _config(D * ln) + (op, "bwd" if bwd else "fwd")


def _cases():
    """(row, op, lhs, rhs, shape).  A "backward only" dot shape reaches the per-edge kernels
    through its gradients alone, so it rotates over the four pairs with an edge operand."""
    cases, gi = [], 0
    edge_pairs = [i for i, p in enumerate(PAIRS) if "e" in p]
    for row, widths, dots in TABLE:
        for kind, shape in [("ew", (w,)) for w in widths] + [("dot", s) for s in dots]:
            for oi, op in enumerate(OPS4 if kind == "ew" else ("dot",)):
                k = gi + oi
                if row == "lane":
                    picks = (k % 3, k % 3 + 3)
                elif row == "bwd_only" and kind == "dot":
                    picks = (edge_pairs[k % 4],)
                else:
                    picks = (k % 6,)
                cases += [(row, op) + PAIRS[p] + (shape,) for p in picks]
            gi += 1
    return cases


def _copy_widths():
    return [w for _, widths, _ in TABLE for w in widths if _supported("use_lhs", False, w, 1)]


def _swapped(op, lhs, rhs):
    return op in ("add", "mul") and CODE[lhs] > CODE[rhs]


def _coverage(cases):
    """Every instance of kernels_sddmm.hip is reached, every target pair meets every op on a
    lane and on a group width in the swapped and the unswapped kind, both gradients (want 0
    and 1) and the gate from both sides."""
    assert len(set(cases)) == len(cases)
    reached, met, wants = set(), set(), set()
    for row, op, lhs, rhs, shape in cases:
        f, b = _instance(op, shape, False), _instance(op, shape, True)
        assert (f is None, b is None) == {"bwd_only": (op == "dot", False),
                                          "neither": (True, True)}.get(row, (False, False)), (row, op, shape)
        if row in ("lane", "group"):
            assert f[0] == row
        if row == "bwd_only" and op == "dot":  # its gradients are all it runs in these kernels
            assert "e" in (lhs, rhs) and b[0] == "group", (op, lhs, rhs, shape)
        if f:
            reached.add(f)
            met.add((f[0], (lhs, rhs), op, _swapped(op, lhs, rhs)))
        if b and "e" in (lhs, rhs):
            reached.add(b)
            want = 0 if lhs == "e" else 1
            wants.add((b[0], b[2], 1 - want if _swapped(op, lhs, rhs) else want))
    for w in _copy_widths():
        reached.add(_config(w) + ("use_lhs", "fwd"))
        reached.add(_config(w) + ("use_lhs", "bwd"))
    expect = set()
    for d in ("fwd", "bwd"):
        for op in OPS:
            expect |= {("lane", nf, op, d) for nf in (1, 2, 3, 4, 6, 8) if not (op == "dot" and nf == 1)}
            expect |= {("group", cfg, op, d) for cfg in GROUP_CFGS}
    assert reached == expect, (sorted(map(str, expect - reached)), sorted(map(str, reached - expect)))
    for kernel in ("lane", "group"):
        for pair in PAIRS:
            for op in OPS4 + ("dot",):
                swap = _swapped(op, *pair)
                assert (kernel, pair, op, swap) in met, (kernel, pair, op)
        kinds = {(op, sw) for k, _, op, sw in met if k == kernel}
        assert kinds == {(op, False) for op in OPS4 + ("dot",)} | {("add", True), ("mul", True)}
        # roles exchanged without a swap: v_sub_u, e_div_u, v_dot_u, ...
        assert {(op, p) for k, p, op, sw in met if k == kernel and not sw and CODE[p[0]] > CODE[p[1]]} \
            >= {(op, p) for op in ("sub", "div", "dot") for p in (("v", "u"), ("e", "v"), ("e", "u"))}
        # after the swap the edge operand of add / mul is always the rhs: want 1 only
        assert {(op, w) for k, op, w in wants if k == kernel} \
            == {(op, w) for op in OPS4 + ("dot",) for w in (0, 1) if w or op not in ("add", "mul")}


CASES = _cases()
_coverage(CASES)


def _case_id(c):
    row, op, lhs, rhs, shape = c
    return "%s-%s_%s_%s-%s" % (row, lhs, op, rhs, "x".join(map(str, shape)))


def _seed(*key):
    return zlib.crc32(repr(key).encode()) % (2 ** 31)


def _feats(rs, rows, shape, away_from_zero=False):
    x = rs.uniform(-1, 1, (rows,) + tuple(shape))
    if away_from_zero:  # a divisor: magnitude in [0.5, 1.5], random sign
        x = (np.abs(x) + 0.5) * np.where(x < 0, -1.0, 1.0)
    return x.astype(np.float32)


class Graph:
    def __init__(self, src, dst, n):
        self.src, self.dst, self.n, self.m = np.asarray(src), np.asarray(dst), n, len(src)
        self.g = dgl.DGLGraph()
        self.g.add_nodes(n)
        self.g.add_edges(self.src, self.dst)
        self.gidx = self.g._graph.get_immutable_gidx(DEV)
        self.rows = {"u": n, "v": n, "e": self.m}

    def ends(self, t):
        return {"u": self.src, "v": self.dst, "e": np.arange(self.m)}[t]


_MAIN = []


def main_graph():
    if not _MAIN:
        src, dst, n = powerlaw(500, 6001, seed=7)
        deg = np.bincount(dst, minlength=n)
        pairs = np.unique(np.stack([src, dst]), axis=1).shape[1]
        assert len(src) % 4 == 1 and (deg == 0).any() and pairs < len(src)  # tails, empty rows, duplicates
        _MAIN.append(Graph(src, dst, n))
    return _MAIN[0]


@contextlib.contextmanager
def sddmm_order(order):
    K.set_sddmm_order(order)
    try:
        yield
    finally:
        K.set_sddmm_order("auto")


def _dev(a):
    return th.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nan(*shape):
    return th.full(tuple(shape), float("nan"), device=DEV)


def _same_bits(a, b):
    return bool(th.equal(a.view(th.int32), b.view(th.int32)))


def _equal(got, want, tag):
    """Finite, then equal as floats (np.array_equal: +-0 are one value)."""
    got = np.asarray(got).reshape(want.shape)
    finite = np.isfinite(got)
    assert finite.all(), "%s: %d of %d not finite (left unwritten?)" % (tag, int((~finite).sum()), got.size)
    if not np.array_equal(got, want):
        bad = got != want
        rows = np.unique(np.nonzero(bad)[0])
        raise AssertionError("%s: %d of %d elements differ (rows %s ...), max |diff| %g" % (
            tag, int(bad.sum()), bad.size, rows[:6].tolist(), float(np.abs(got - want).max())))


def _shapes(op, shape):
    return (tuple(shape), tuple(shape[:-1]) if op == "dot" else tuple(shape))


def _inputs(G, case):
    _, op, lhs, rhs, shape = case
    rng = np.random.RandomState(_seed(case))
    lv = _feats(rng, G.rows[lhs], shape)
    rv = _feats(rng, G.rows[rhs], shape, away_from_zero=op == "div")
    oshape = _shapes(op, shape)[1]
    go = {"none": rng.uniform(-1, 1, (G.m,) + oshape).astype(np.float32),
          "sum": rng.uniform(-1, 1, (G.n,) + oshape).astype(np.float32)}
    return lv, rv, go


def run_forward(gidx, m, op, lhs, rhs, lt, rt):
    out = _nan(m, *_shapes(op, lt.shape[1:])[1])
    K.binary_op_reduce("none", op, gidx, CODE[lhs], CODE[rhs], lt, rt, out)
    return out


def run_backward(gidx, red, op, lhs, rhs, lt, rt, got):
    """(grad_lhs, grad_rhs) in the kernel's shape.  Reducers none / sum do not read the
    forward output: it is passed as zeros of the right shape."""
    out = th.zeros_like(got)
    gl, gr = _nan(*lt.shape), _nan(*rt.shape)
    K.backward_lhs_binary_op_reduce(red, op, gidx, CODE[lhs], CODE[rhs], lt, rt, out, got, gl)
    K.backward_rhs_binary_op_reduce(red, op, gidx, CODE[lhs], CODE[rhs], lt, rt, out, got, gr)
    return gl, gr


def both_orders(run, tag):
    """run() in edge-id order and in in-CSR order, twice each: four bit-equal results (a
    tuple of device tensors); returns the first on the host."""
    res = []
    for order in ("coo", "csr"):
        with sddmm_order(order):
            res += [run(), run()]
    for i, name in ((1, "coo twice"), (2, "coo / csr"), (3, "csr twice")):
        assert all(_same_bits(a, b) for a, b in zip(res[0], res[i])), "%s: %s differ" % (tag, name)
    return [x.cpu().numpy() for x in res[0]]


def expected_forward(op, shape, L, Rr, t):
    """(fp32 value, checked against fp64 too?)."""
    if op == "dot" and _instance(op, shape, False) and _config(shape[0] * shape[1])[0] == "group" \
            and shape[1] > 1:
        return R.dot_group32(L, Rr), True
    return t.e32, False


def check_forward(op, shape, L, Rr, t, got, tag):
    want, bound = expected_forward(op, shape, L, Rr, t)
    _equal(got, want, tag)
    if bound:
        R.assert_within(got, t.e64, (shape[1] + 1) * R.EPS * t.emaj, tag + " vs fp64")


def check_grads(G, case, L, Rr, t, go_e, got, tag):
    """got = (grad_lhs, grad_rhs) of one reducer, go_e grad_out at each edge's output row."""
    _, op, lhs, rhs, shape = case
    ln = _dims(op, shape)[1]
    gl, glmaj, gr, grmaj = R.edge_grads("sum", t, go_e)
    g32 = R.edge_grads32(op, L, Rr, go_e)
    on_sddmm = _instance(op, shape, True) is not None
    for w, (tgt, g, gmaj) in enumerate(((lhs, gl, glmaj), (rhs, gr, grmaj))):
        name = "%s grad %s" % (tag, ("lhs", "rhs")[w])
        if tgt == "e":
            if on_sddmm:
                _equal(got[w], g32[w], name)
                R.assert_within(got[w], g, R.edge_bound(gmaj, 0), name + " vs fp64")
            else:
                R.assert_within(got[w], g, R.edge_bound(gmaj, ln), name)
        else:
            exact, mass = R.scatter_sum(g, gmaj, G.ends(tgt), G.n)
            deg = np.bincount(G.ends(tgt), minlength=G.n)
            R.assert_within(got[w], exact, R.node_sum_bound(mass, deg.reshape((-1,) + (1,) * (g.ndim - 1)), ln), name)
            assert (got[w][deg == 0] == 0).all(), name + ": rows without terms"


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_instances(case):
    """Forward, and with an edge operand both gradients under reducers none and sum, in both
    item orders."""
    _, op, lhs, rhs, shape = case
    G = main_graph()
    lv, rv, go = _inputs(G, case)
    lt, rt = _dev(lv), _dev(rv)
    L, Rr = lv[G.ends(lhs)], rv[G.ends(rhs)]
    t = R.EdgeTerms(op, L, Rr)
    tag = _case_id(case)
    out, = both_orders(lambda: (run_forward(G.gidx, G.m, op, lhs, rhs, lt, rt),), tag + " forward")
    check_forward(op, shape, L, Rr, t, out, tag + " forward")
    if "e" not in (lhs, rhs):
        return
    for red in ("none", "sum"):
        got = _dev(go[red])
        grads = both_orders(lambda: run_backward(G.gidx, red, op, lhs, rhs, lt, rt, got),
                            "%s %s" % (tag, red))
        check_grads(G, case, L, Rr, t, go[red] if red == "none" else go[red][G.dst], grads,
                    "%s %s" % (tag, red))


@pytest.mark.parametrize("width", _copy_widths())
def test_copy(width):
    """copy_u / copy_e with reducer none (OP_USE_LHS forward) and the gradient of copy_e under
    reducers sum and none (OP_USE_LHS backward: grad_out at the destination row / the edge)."""
    G = main_graph()
    rng = np.random.RandomState(_seed("copy", width))
    for tgt in ("u", "e"):
        x = _feats(rng, G.rows[tgt], (width,))
        xt = _dev(x)

        def fwd():
            out = _nan(G.m, width)
            K.copy_reduce("none", G.gidx, CODE[tgt], xt, out)
            return (out,)
        out, = both_orders(fwd, "copy_%s %d" % (tgt, width))
        _equal(out, x[G.ends(tgt)], "copy_%s %d" % (tgt, width))
    for red, rows, at in (("sum", G.n, G.dst), ("none", G.m, np.arange(G.m))):
        go = rng.uniform(-1, 1, (rows, width)).astype(np.float32)
        got, outbuf = _dev(go), th.zeros(rows, width, device=DEV)

        def bwd():
            grad = _nan(G.m, width)
            K.backward_copy_reduce(red, G.gidx, CODE["e"], xt, outbuf, got, grad)
            return (grad,)
        grad, = both_orders(bwd, "copy_e %s backward %d" % (red, width))
        _equal(grad, go[at], "copy_e %s backward %d" % (red, width))


# ---- further cases at NF 6, 12, 260 and dot (2, 512) ----------------------------------------
EXTRA = (("sub", "e", "v", (6,)), ("div", "u", "e", (12,)), ("mul", "e", "u", (260,)),
         ("dot", "v", "e", (2, 512)))
_extra_id = lambda c: "%s_%s_%s-%s" % (c[1], c[0], c[2], "x".join(map(str, c[3])))


def _off4(a):
    """A contiguous device copy of ``a`` that starts 4 bytes into its storage."""
    base = th.empty(a.size + 1, dtype=th.float32, device=DEV)
    view = base[1:].view(a.shape)
    view.copy_(th.from_numpy(a))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("c", EXTRA, ids=_extra_id)
def test_alignment_gate(c):
    """Operands, grad_out and outputs 4 bytes off 16-byte alignment: the entry must take the
    generic kernels (scalar accesses), not the float4 / float2 ones.  Elementwise results
    equal the aligned call's; the dot is the generic kernels' sequential one (which the
    aligned call's group order is not) and the gradients keep the generic bound.  On the dot
    the forward also runs with one buffer unaligned at a time."""
    op, lhs, rhs, shape = c
    case = ("extra",) + c
    G = main_graph()
    lv, rv, go = _inputs(G, case)
    L, Rr = lv[G.ends(lhs)], rv[G.ends(rhs)]
    t = R.EdgeTerms(op, L, Rr)
    full, oshape = _shapes(op, shape)
    tag = "unaligned " + _extra_id(c)

    def run(off):
        put = _off4 if off else _dev
        blank = (lambda *s: _off4(np.full(s, np.nan, np.float32))) if off else _nan
        lt, rt, got = put(lv), put(rv), put(go["none"])
        out = blank(G.m, *oshape)
        K.binary_op_reduce("none", op, G.gidx, CODE[lhs], CODE[rhs], lt, rt, out)
        zeros = put(np.zeros((G.m,) + oshape, np.float32))
        gl, gr = blank(*lv.shape), blank(*rv.shape)
        K.backward_lhs_binary_op_reduce("none", op, G.gidx, CODE[lhs], CODE[rhs], lt, rt, zeros, got, gl)
        K.backward_rhs_binary_op_reduce("none", op, G.gidx, CODE[lhs], CODE[rhs], lt, rt, zeros, got, gr)
        return [x.cpu().numpy() for x in (out, gl, gr)]
    aligned, off = run(False), run(True)
    _equal(off[0], t.e32, tag + " forward")
    if op == "dot":
        assert (aligned[0] != off[0]).mean() > 0.25, tag + ": the aligned call's order"
        R.assert_within(off[0], t.e64, (shape[1] + 1) * R.EPS * t.emaj, tag + " forward vs fp64")
        # one buffer off at a time: each term of the forward's gate alone sends the call to
        # the generic kernels, which the sequential order shows
        for which in ("lhs", "rhs", "out"):
            lt = (_off4 if which == "lhs" else _dev)(lv)
            rt = (_off4 if which == "rhs" else _dev)(rv)
            out = _off4(np.full((G.m,) + oshape, np.nan, np.float32)) if which == "out" else _nan(G.m, *oshape)
            K.binary_op_reduce("none", op, G.gidx, CODE[lhs], CODE[rhs], lt, rt, out)
            _equal(out.cpu().numpy(), t.e32, "%s forward, only %s unaligned" % (tag, which))
    else:
        _equal(off[0], aligned[0], tag + " forward vs aligned")
    w = 0 if lhs == "e" else 1
    gl, glmaj, gr, grmaj = R.edge_grads("sum", t, go["none"])
    R.assert_within(off[1 + w], (gl, gr)[w], R.edge_bound((glmaj, grmaj)[w], _dims(op, shape)[1]),
                    tag + " edge gradient")
    _equal(off[1 + w], aligned[1 + w], tag + " edge gradient vs aligned")


@pytest.mark.parametrize("c", EXTRA, ids=_extra_id)
def test_wide_index_layout(c):
    """asbits(64): int64 offsets and edge ids, read through the wide IdxPtr in in-CSR order;
    bit-equal to the int32 layout, forward and both gradients under both reducers."""
    op, lhs, rhs, shape = c
    G = main_graph()
    g64 = G.g._graph.asbits(64).get_immutable_gidx(DEV)
    assert g64.in_csr.data.dtype == th.int64 and G.gidx.in_csr.data.dtype == th.int32
    lv, rv, go = _inputs(G, ("extra",) + c)
    lt, rt = _dev(lv), _dev(rv)
    with sddmm_order("csr"):
        for gidx in (G.gidx, g64):
            res = [run_forward(gidx, G.m, op, lhs, rhs, lt, rt)]
            for red in ("none", "sum"):
                res += run_backward(gidx, red, op, lhs, rhs, lt, rt, _dev(go[red]))
            if gidx is G.gidx:
                base = res
    assert all(bool(th.isfinite(x).all()) for x in res)
    assert all(_same_bits(a, b) for a, b in zip(base, res)), _extra_id(c)


PARTIAL = (("mul", "u", "e", (6,)), ("sub", "e", "v", (12,)), ("div", "v", "e", (260,)),
           ("dot", "e", "u", (2, 512)))


@pytest.mark.parametrize("c", PARTIAL, ids=_extra_id)
def test_partial_apply_edges(c):
    """apply_edges on every third edge: a parent-eid subgraph, items in in-CSR positions, edge
    ids no permutation.  Touched rows equal the restatement, untouched rows keep a sentinel."""
    op, lhs, rhs, shape = c
    M = main_graph()
    G = Graph(M.src, M.dst, M.n)  # its own frames
    lv, rv, _ = _inputs(G, ("partial",) + c)
    for t_, v in ((lhs, lv), (rhs, rv)):
        (G.g.edata if t_ == "e" else G.g.ndata)["x" + t_] = _dev(v)
    builtin = getattr(fn, "%s_%s_%s" % (lhs, op, rhs))("x" + lhs, "x" + rhs, "o")
    G.g.apply_edges(builtin)
    whole = G.g.edata["o"]
    L, Rr = lv[G.ends(lhs)], rv[G.ends(rhs)]
    want = R.dot_group32(L, Rr) if op == "dot" else R.EdgeTerms(op, L, Rr).e32
    _equal(whole.cpu().numpy(), want, "apply_edges " + _extra_id(c))
    sub = np.arange(0, G.m, 3)
    G.g.edata["o"] = th.full_like(whole, 7.5)
    G.g.apply_edges(builtin, edges=sub)
    got = G.g.edata["o"].cpu().numpy().reshape(want.shape)
    keep = np.ones(G.m, bool)
    keep[sub] = False
    assert (got[keep] == 7.5).all(), "untouched rows"
    _equal(got[sub], want[sub], "partial apply_edges " + _extra_id(c))


@pytest.mark.parametrize("edges", [1, 2, 3, 5])
@pytest.mark.parametrize("op,shape", [("add", (12,)), ("div", (260,)), ("dot", (3, 4)), ("dot", (65, 4))],
                         ids=["add-12", "div-260", "dot-3x4", "dot-65x4"])
def test_small_edge_counts(edges, op, shape):
    """1, 2, 3 and 5 edges on 4 nodes: the whole launch is a tail (U = 4 at NF 12, U = 2 at
    NF 260)."""
    src = np.array([3, 0, 3, 1, 2])[:edges]
    dst = np.array([1, 1, 2, 3, 1])[:edges]
    G = Graph(src, dst, 4)
    case = ("small%d" % edges, op, "e", "v", shape)
    lv, rv, go = _inputs(G, case)
    lt, rt = _dev(lv), _dev(rv)
    L, Rr = lv[G.ends("e")], rv[G.ends("v")]
    t = R.EdgeTerms(op, L, Rr)
    tag = "%d edges %s %s" % (edges, op, shape)
    out, = both_orders(lambda: (run_forward(G.gidx, G.m, op, "e", "v", lt, rt),), tag)
    check_forward(op, shape, L, Rr, t, out, tag + " forward")
    for red in ("none", "sum"):
        got = _dev(go[red])
        grads = both_orders(lambda: run_backward(G.gidx, red, op, "e", "v", lt, rt, got), tag + red)
        check_grads(G, case, L, Rr, t, go[red] if red == "none" else go[red][G.dst], grads, tag + " " + red)


# ---- grid-stride sweeps --------------------------------------------------------------------
SWEEPS = {"64x4": (65536 + 3, (("mul", (516,)), ("dot", (129, 4)))),
          "64x1": (262144 + 5, (("add", (132,)), ("dot", (33, 4)))),
          "lane": (4194304 + 257, (("add", (1,)), ("add", (8,)), ("mul", (12,))))}
SAMPLE = 70000
SWEEP_RUNS = [(key, i) for key, (_, runs) in SWEEPS.items() for i in range(len(runs))]


@pytest.fixture(scope="module")
def sweep(request):
    """One graph per sweep, alive for its runs only."""
    src, dst, n = powerlaw(1000, SWEEPS[request.param][0], seed=11)
    G = Graph(src, dst, n)
    yield G
    del G
    th.cuda.empty_cache()


@pytest.mark.parametrize("sweep,run", [(k, SWEEPS[k][1][i]) for k, i in SWEEP_RUNS], indirect=["sweep"],
                         ids=["%s-%s-%s" % ((k, SWEEPS[k][1][i][0], "x".join(map(str, SWEEPS[k][1][i][1]))))
                              for k, i in SWEEP_RUNS])
def test_grid_stride(sweep, run):
    """More edges than one sweep of the 16 384-block grid, "auto" order, forward, node
    operands (only the output is large).  Equality on every element; the dot also within its
    fp64 bound on the last 70 000 edges and on a fixed sample of 70 000."""
    G, (op, shape) = sweep, run
    rng = np.random.RandomState(_seed("sweep", G.m, op, shape))
    cfg = _config(int(np.prod(shape)))
    per_sweep = 16384 * (256 if cfg[0] == "lane" else (256 // cfg[1][0]) * {1: 4, 2: 2, 4: 1}[cfg[1][1]])
    assert per_sweep < G.m < 2 * per_sweep and _instance(op, shape, False)
    lv, rv = _feats(rng, G.n, shape), _feats(rng, G.n, shape)
    lt, rt = _dev(lv), _dev(rv)
    out = run_forward(G.gidx, G.m, op, "u", "v", lt, rt)
    again = run_forward(G.gidx, G.m, op, "u", "v", lt, rt)
    assert _same_bits(out, again)
    del again
    out = out.cpu().numpy()
    tag = "%d edges %s %s" % (G.m, op, shape)
    for lo in range(0, G.m, 1 << 19):
        sl = slice(lo, min(G.m, lo + (1 << 19)))
        L, Rr = lv[G.src[sl]], rv[G.dst[sl]]
        want = {"add": lambda: L + Rr, "mul": lambda: L * Rr, "dot": lambda: R.dot_group32(L, Rr)}[op]()
        _equal(out[sl], want, "%s from edge %d" % (tag, lo))
    if op == "dot":
        pick = np.unique(np.concatenate([np.arange(max(0, G.m - SAMPLE), G.m),
                                         rng.choice(G.m, min(SAMPLE, G.m), replace=False)]))
        t = R.EdgeTerms(op, lv[G.src[pick]], rv[G.dst[pick]])
        R.assert_within(out[pick], t.e64, (shape[1] + 1) * R.EPS * t.emaj, tag + " vs fp64")
