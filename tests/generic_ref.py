"""A numpy restatement of binary_op_reduce and its two gradients, for the tests of the
generic kernels (csrc/kernels_generic.hip).  It shares no code with the kernels or with
the C oracle (oracle/dgl_ref.c): everything is whole-array numpy over the edge list.

For an edge j with ends ``end_l[j]`` / ``end_r[j]`` the operands are ``L = lhs[end_l]``
and ``R = rhs[end_r]`` (through ``lhs_map`` / ``rhs_map`` when given: ``lhs[lhs_map[id]]``).
Their feature shapes broadcast like numpy's, right-aligned, the missing size-1 dims
inserted after the edge dim; ``dot`` contracts the last dim.

Three versions of every per-edge value:

* fp32, restating the kernel's arithmetic (one IEEE operation per element for add / sub /
  mul / div; ``acc = 0; acc = acc + l[i] * r[i]`` for dot, in that order, each operation
  rounded).  These define max / min, reducer "none" and the tie mask ``e == out[dst]``;
* fp64, the same expressions, for sums and gradients;
* a majorant: the fp64 expression with every operand replaced by its absolute value and
  every subtraction by an addition.  An fp32 evaluation with k roundings is within
  k * 2^-24 * majorant of the fp64 value (to first order), whatever the order of a sum.

For the per-edge kernels (csrc/kernels_sddmm.hip) two more fp32 restatements: the group
kernel's dot in its own order (``dot_group32``) and the per-edge gradients
(``edge_grads32``).

Gradients come in the shape the kernel writes (the full broadcast shape, dot length
included) and, like ``dgl.backend._reduce_grad``, summed down to the operand's shape.
"""
import numpy as np

EPS = 2.0 ** -24
FLT_MAX = np.float32(3.402823466e38)
IDENTITY = {"sum": np.float32(0), "none": np.float32(0), "max": -FLT_MAX, "min": FLT_MAX,
            "prod": np.float32(1)}


def feature_shapes(op, lshape, rshape):
    """(lhs padded, rhs padded, full, out, len): ``full`` is the broadcast feature shape
    (a gradient's, with the dot length last), ``out`` the forward output's."""
    nd = max(len(lshape), len(rshape))
    lp = (1,) * (nd - len(lshape)) + tuple(lshape)
    rp = (1,) * (nd - len(rshape)) + tuple(rshape)
    full = tuple(np.broadcast_shapes(lp, rp))
    if op == "dot":
        assert lp[-1] == rp[-1]
        return lp, rp, full, full[:-1], full[-1]
    return lp, rp, full, full, 1


class EdgeTerms:
    """Per-edge values of ``op`` and its partial derivatives for L (m,) + lshape and
    R (m,) + rshape (fp32): e32, e64, emaj of shape (m,) + out; dl, dr (fp64) and dlmaj,
    drmaj of shape (m,) + full."""

    def __init__(self, op, L, R):
        m = L.shape[0]
        lp, rp, full, out, ln = feature_shapes(op, L.shape[1:], R.shape[1:])
        self.op, self.m, self.full, self.out, self.len = op, m, full, out, ln
        L = L.reshape((m,) + lp).astype(np.float32)
        R = R.reshape((m,) + rp).astype(np.float32)
        L64, R64 = L.astype(np.float64), R.astype(np.float64)
        aL, aR = np.abs(L64), np.abs(R64)
        one = np.ones((m,) + full)
        if op == "use_lhs":  # copy: R is ignored (pass L)
            self.e32, self.e64, self.emaj = L, L64, aL
            self.dl, self.dr, self.dlmaj, self.drmaj = one, 0 * one, one, 0 * one
        elif op == "dot":
            acc = np.zeros((m,) + out, np.float32)
            for i in range(ln):
                acc = acc + L[..., i] * R[..., i]
            self.e32 = acc
            self.e64 = (L64 * R64).sum(-1)
            self.emaj = (aL * aR).sum(-1)
            self.dl, self.dr = R64 * one, L64 * one
            self.dlmaj, self.drmaj = aR * one, aL * one
        elif op == "add":
            self.e32, self.e64, self.emaj = L + R, L64 + R64, aL + aR
            self.dl, self.dr, self.dlmaj, self.drmaj = one, one, one, one
        elif op == "sub":
            self.e32, self.e64, self.emaj = L - R, L64 - R64, aL + aR
            self.dl, self.dr, self.dlmaj, self.drmaj = one, -one, one, one
        elif op == "mul":
            self.e32, self.e64, self.emaj = L * R, L64 * R64, aL * aR
            self.dl, self.dr = R64 * one, L64 * one
            self.dlmaj, self.drmaj = aR * one, aL * one
        elif op == "div":
            self.e32, self.e64, self.emaj = L / R, L64 / R64, aL / aR
            self.dl, self.dr = (1 / R64) * one, (-L64 / (R64 * R64)) * one
            self.dlmaj, self.drmaj = (1 / aR) * one, (aL / (aR * aR)) * one
        else:
            raise ValueError(op)
        assert self.e32.dtype == np.float32 and self.e32.shape == (m,) + out


def dot_group32(L, R):
    """The dot of k_sddmm_group (csrc/kernels_sddmm.hip) in its own order, fp32 with every
    operation rounded, for L, R of shape (m, D, len), len % 4 == 0 and S = len / 4 a power of
    two: the products; per float4 ((x + y) + z) + w; a balanced pairwise tree over
    min(S, 64) adjacent float4, adjacent pairs first (what the xor butterfly leaves in the
    lowest lane of a segment); for S > 64, acc = 0; acc = acc + part[v] over the S / 64 slots
    in order.  Returns (m, D)."""
    L, R = np.asarray(L, np.float32), np.asarray(R, np.float32)
    m, D, ln = L.shape
    S = ln // 4
    assert L.shape == R.shape and ln % 4 == 0 and S > 0 and S & (S - 1) == 0
    p = (L * R).reshape(m, D, S, 4)
    part = ((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]
    span = min(S, 64)
    part = part.reshape(m, D, S // span, span)
    while part.shape[-1] > 1:
        part = part[..., 0::2] + part[..., 1::2]
    part = part[..., 0]
    if S <= 64:
        out = part[..., 0]
    else:
        out = np.zeros((m, D), np.float32)
        for v in range(S // span):
            out = out + part[..., v]
    assert out.dtype == np.float32
    return out


def edge_grads32(op, L, R, ge):
    """The per-edge gradients (gl, gr) in fp32 as the per-edge kernels compute them (bwd1 of
    kernels_sddmm.hip with op_grad_lhs / op_grad_rhs of internal.h), each operation rounded in
    this order: add ge, ge; sub ge, ge * -1; mul and dot ge * r, ge * l; div ge * (1 / r),
    ge * (-l / (r * r)); use_lhs ge, None.  L, R (m,) + full (R ignored for use_lhs), ge
    (m,) + out: for dot the length dim is missing and ge is repeated over it."""
    L = np.asarray(L, np.float32)
    ge = np.asarray(ge, np.float32)
    if op == "dot":
        ge = np.broadcast_to(ge.reshape(L.shape[:-1])[..., None], L.shape)
    else:
        ge = ge.reshape(L.shape)
    if op == "use_lhs":
        return ge.copy(), None
    R = np.asarray(R, np.float32)
    assert L.shape == R.shape
    one = np.float32(1)
    if op == "add":
        gl, gr = ge * one, ge * one
    elif op == "sub":
        gl, gr = ge * one, ge * -one
    elif op in ("mul", "dot"):
        gl, gr = ge * R, ge * L
    elif op == "div":
        gl, gr = ge * (one / R), ge * (-L / (R * R))
    else:
        raise ValueError(op)
    assert gl.dtype == np.float32 and gr.dtype == np.float32
    return gl, gr


def _flat(a):
    return a.reshape(a.shape[0], -1)


def _fold_rows(ufunc, vals, rows, n, fill, dtype):
    """out[r] = ufunc-fold of vals[j] over the edges j with rows[j] == r, in edge order;
    rows without edges keep ``fill``."""
    flat = _flat(vals)
    out = np.full((n, flat.shape[1]), fill, dtype)
    if flat.shape[0]:
        order = np.argsort(rows, kind="stable")
        present, start = np.unique(np.asarray(rows)[order], return_index=True)
        out[present] = ufunc.reduceat(flat[order], start, axis=0)
    return out.reshape((n,) + vals.shape[1:])


def scatter_sum(vals, maj, rows, n):
    """(exact, mass), each (n,) + vals.shape[1:]: per-row fp64 sums of vals and of maj."""
    return (_fold_rows(np.add, vals.astype(np.float64), rows, n, 0.0, np.float64),
            _fold_rows(np.add, maj.astype(np.float64), rows, n, 0.0, np.float64))


def reduce_forward(red, t, rows, n):
    """The forward output over n rows (row of edge j: rows[j]).  sum: (exact, mass) in
    fp64; prod: (exact, None); max / min: (out32, None), the fp32 fold of t.e32 from the
    identity -- empty rows keep it."""
    if red == "sum":
        return scatter_sum(t.e64, t.emaj, rows, n)
    if red == "prod":
        return _fold_rows(np.multiply, t.e64, rows, n, 1.0, np.float64), None
    fold = np.maximum if red == "max" else np.minimum
    return _fold_rows(fold, t.e32, rows, n, IDENTITY[red], np.float32), None


def edge_grads(red, t, go_e, out_e=None):
    """Per-edge gradients in the full shape: (gl, glmaj, gr, grmaj), each (m,) + full.
    go_e (m,) + out: grad_out at the edge's output row (at the edge for "none").  out_e:
    the forward output at that row -- fp32 for max / min (the tie mask t.e32 == out_e,
    every tied edge gets the gradient), fp64 for prod (out / e)."""
    ge = go_e.reshape((t.m,) + t.out).astype(np.float64)
    if red in ("max", "min"):
        ge = ge * (t.e32 == out_e.reshape(ge.shape))
        gemaj = np.abs(ge)
    elif red == "prod":
        f = out_e.reshape(ge.shape) / t.e64
        ge, gemaj = ge * f, np.abs(ge) * np.abs(f)
    else:
        gemaj = np.abs(ge)
    if t.op == "dot":
        ge, gemaj = ge[..., None], gemaj[..., None]
    return ge * t.dl, gemaj * t.dlmaj, ge * t.dr, gemaj * t.drmaj


def reduce_to(a, shape):
    """Sum ``a`` (rows,) + full over the dims that ``shape`` (an operand's feature shape)
    broadcasts, as _reduce_grad does.  Returns the reduced array and the largest number of
    elements summed into one."""
    full = a.shape[1:]
    pad = (1,) * (len(full) - len(shape)) + tuple(shape)
    axes = tuple(i + 1 for i, (f, s) in enumerate(zip(full, pad)) if f != s)
    if not axes:
        return a.reshape((a.shape[0],) + tuple(shape)), 1
    k = int(np.prod([full[i - 1] for i in axes]))
    return a.sum(axis=axes, keepdims=True).reshape((a.shape[0],) + tuple(shape)), k


def through(table, ids, id_map=None):
    """operand[map[id]] on reads."""
    return table[ids if id_map is None else id_map[ids]]


def place(rows_total, values, row_map, fill):
    """out[out_map[row]] on writes: ``values`` (k,) + feat placed at row_map[i] of a table
    of rows_total rows filled with ``fill``; untouched rows keep the fill."""
    out = np.full((rows_total,) + values.shape[1:], fill, values.dtype)
    out[np.arange(values.shape[0]) if row_map is None else row_map] = values
    return out


def assert_within(got, exact, bound, tag):
    """Every element of got is finite and within bound of exact.  A NaN -- an element a
    kernel left unwritten in a NaN-filled buffer, or computed as one -- fails: it is
    rejected first, and the comparison is written so that it could not pass anyway."""
    got = np.asarray(got).astype(np.float64).reshape(exact.shape)
    finite = np.isfinite(got)
    assert finite.all(), "%s: %d of %d not finite (left unwritten?)" % (
        tag, int((~finite).sum()), got.size)
    err = np.abs(got - exact)
    bad = ~(err <= bound)
    assert not bad.any(), "%s: %d of %d outside, max excess %g (err %g)" % (
        tag, int(bad.sum()), bad.size, float(np.nanmax(err - bound)), float(np.nanmax(err)))


def node_sum_bound(mass, deg, ln):
    """The suite's bound for an fp32 node-owned sum (test_generic_gpu._check_node_sum) with
    the dot length added to the chain.  deg: per-row term counts, shaped to broadcast."""
    return 1e-4 + (512 + deg / 128.0 + ln + 2) * EPS * mass


def edge_bound(maj, ln, extra=0):
    """Per-edge gradients: at most six fp32 roundings around a len-term dot (``extra``
    more for a sum over ``extra + 1`` elements taken afterwards)."""
    return (ln + 6 + extra) * EPS * maj
