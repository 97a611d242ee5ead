"""Segment kernels (DGLMISegment*) and the readout functions over dgl.batch, on the GPU.

Segment length lists are built around the walk's chunk R = kernel.segment_chunk_rows(F):
empty segments first, in the middle and last, segments of R - 1, R and R + 1 rows, one
segment over more than kFixSeg = 32 chunks (the segmented fixup), a thousand one-row
segments, one segment (an unbatched graph) and no segment at all; at every slot width and
lane layout (F = 1 .. 1028).  The reference is numpy on the CPU, per segment, in float64.

Exact checks use integer features in [-8, 8] and weights in [-4, 4]: every fp32 partial
sum is exact in any order, so results must be equal, not close.  The float checks use the
bound of fp32 summation in any order plus one product rounding,
|err| <= 1.01 (n + 2) 2^-24 sum|w x|.
"""
import numpy as np
import pytest
import torch as th

import dgl
from dgl import backend as B
from dgl import kernel as K

pytestmark = pytest.mark.gpu
DEV = th.device("cuda:0")
FS = [1, 2, 3, 4, 5, 64, 65, 1028]
CASES = ["edges", "ones", "single", "none"]
U = 2.0 ** -24


def _lens(case, F):
    R = K.segment_chunk_rows(F)
    assert R >= 16 and R % 16 == 0
    if case == "edges":
        return [0, 1, R - 1, R, R + 1, 0, 0, 3, 33 * R + 5, 0]
    if case == "ones":
        return [1] * 1000
    if case == "single":
        return [2 * R + 3]
    return []


def _seg(lens):
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(np.asarray(lens, np.int64), out=off[1:])
    return K.Segments(th.from_numpy(off).to(DEV), int(off[-1])), off


def _ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


def _per_segment(fn, x, off, empty):
    """fn over the rows of every segment of x (float64), `empty` for one without rows."""
    out = np.empty((len(off) - 1,) + x.shape[1:], np.float64)
    for b in range(len(off) - 1):
        rows = x[off[b]:off[b + 1]]
        out[b] = fn(rows) if len(rows) else empty
    return out


def _seg_ids(off):
    return np.repeat(np.arange(len(off) - 1), np.diff(off))


def _t(a):
    return th.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _twice(fn):
    a, b = fn(), fn()
    for u, v in zip(a, b):
        assert th.equal(u, v), "two launches differ"
    return a


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("case", CASES)
def test_sum_mean_weighted_exact(case, F):
    lens = _lens(case, F)
    seg, off = _seg(lens)
    n, nb = int(off[-1]), len(lens)
    rng = np.random.default_rng(F * 7 + len(lens))
    x, w = _ints(rng, (n, F), -8, 8), _ints(rng, (n,), -4, 4)
    gy = _ints(rng, (nb, F), -4, 4)
    sid = _seg_ids(off)
    cnt = np.maximum(np.diff(off), 1).astype(np.float32)

    def run():
        xt, wt = _t(x).requires_grad_(), _t(w).requires_grad_()
        s = B.segment_reduce("sum", seg, xt)
        m = B.segment_reduce("mean", seg, xt)
        ws = B.segment_reduce("sum", seg, xt, wt)
        gs, = th.autograd.grad(s, xt, _t(gy))
        gm, = th.autograd.grad(m, xt, _t(gy))
        gwx, gww = th.autograd.grad(ws, (xt, wt), _t(gy))
        return s.detach(), m.detach(), ws.detach(), gs, gm, gwx, gww

    s, m, ws, gs, gm, gwx, gww = _twice(run)
    x64 = x.astype(np.float64)
    exact = _per_segment(lambda r: r.sum(0), x64, off, 0.0).astype(np.float32)
    assert th.equal(s.cpu(), th.from_numpy(exact))
    assert th.equal(m.cpu(), th.from_numpy(exact) / th.from_numpy(cnt)[:, None])
    wexact = _per_segment(lambda r: r.sum(0), x64 * w[:, None], off, 0.0).astype(np.float32)
    assert th.equal(ws.cpu(), th.from_numpy(wexact))
    # closed forms: d sum / dx = gy[seg], d mean / dx = gy[seg] / n, weighted: gy[seg] w and <x, gy[seg]>
    assert th.equal(gs.cpu(), th.from_numpy(gy[sid]))
    assert th.equal(gm.cpu(), th.from_numpy(gy[sid]) / th.from_numpy(cnt[sid])[:, None])
    assert th.equal(gwx.cpu(), th.from_numpy(gy[sid] * w[:, None]))
    assert th.equal(gww.cpu(), th.from_numpy((x64 * gy[sid]).sum(1).astype(np.float32)))


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("case", CASES)
def test_max_min_exact(case, F):
    lens = _lens(case, F)
    seg, off = _seg(lens)
    n, nb = int(off[-1]), len(lens)
    rng = np.random.default_rng(F * 11 + len(lens))
    x = _ints(rng, (n, F), -8, 8)  # 17 values: long segments tie in every column
    gy = _ints(rng, (nb, F), -4, 4)
    for red, np_red, np_arg, ident in (("max", np.max, np.argmax, -np.inf),
                                       ("min", np.min, np.argmin, np.inf)):
        def run():
            out = th.empty((nb, F), device=DEV)
            arg = th.empty((nb, F), dtype=th.int64, device=DEV)
            K.segment_reduce(red, seg, _t(x), None, out, arg)
            xt = _t(x).requires_grad_()
            y = B.segment_reduce(red, seg, xt)
            g, = th.autograd.grad(y, xt, _t(gy))
            return out, arg, y.detach(), g

        out, arg, y, g = _twice(run)
        ref = _per_segment(lambda r: np_red(r, 0), x, off, ident).astype(np.float32)
        rarg = np.full((nb, F), -1, np.int64)
        for b in range(nb):
            if off[b + 1] > off[b]:
                rarg[b] = off[b] + np_arg(x[off[b]:off[b + 1]], 0)
        assert th.equal(out.cpu(), th.from_numpy(ref))
        assert th.equal(y.cpu(), th.from_numpy(ref))
        assert th.equal(arg.cpu(), th.from_numpy(rarg))
        # the gradient lands on the first row that attains the value, 0 elsewhere
        gref = np.zeros((n, F), np.float32)
        for b in range(nb):
            if off[b + 1] > off[b]:
                gref[rarg[b], np.arange(F)] = gy[b]
        assert th.equal(g.cpu(), th.from_numpy(gref))


def test_max_ties_in_every_column():
    F = 64
    R = K.segment_chunk_rows(F)
    lens = [5, 3 * R + 7, 0, 2]
    seg, off = _seg(lens)
    x = np.ones((int(off[-1]), F), np.float32)  # every row ties
    out = th.empty((4, F), device=DEV)
    arg = th.empty((4, F), dtype=th.int64, device=DEV)
    K.segment_reduce("max", seg, _t(x), None, out, arg)
    assert th.equal(arg.cpu(), th.tensor([[0], [5], [-1], [off[3]]]).expand(4, F))
    xt = _t(x).requires_grad_()
    B.segment_reduce("max", seg, xt).backward(th.ones(4, F, device=DEV))
    g = np.zeros_like(x)
    g[[0, 5, off[3]]] = 1
    assert th.equal(xt.grad.cpu(), th.from_numpy(g))


@pytest.mark.parametrize("F", [1, 4, 65])
def test_max_nan_after_a_larger_value(F):
    R = K.segment_chunk_rows(F)
    lens = [R + 9, 4, 2 * R]
    seg, off = _seg(lens)
    rng = np.random.default_rng(F)
    x = _ints(rng, (int(off[-1]), F), -8, 8)
    x[3], x[7], x[R + 3] = 100.0, np.nan, np.nan  # segment 0: a NaN after a larger finite value
    x[off[2] + R + 1, 0] = np.nan                 # segment 2: in its second chunk
    out = th.empty((3, F), device=DEV)
    arg = th.empty((3, F), dtype=th.int64, device=DEV)
    K.segment_reduce("max", seg, _t(x), None, out, arg)
    ref = np.stack([np.max(x[off[b]:off[b + 1]], 0) for b in range(3)])
    rarg = np.stack([off[b] + np.argmax(x[off[b]:off[b + 1]], 0) for b in range(3)])
    assert np.isnan(ref[0]).all() and rarg[0, 0] == 7
    assert np.array_equal(out.cpu().numpy(), ref, equal_nan=True)
    assert th.equal(arg.cpu(), th.from_numpy(rarg))


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("case", CASES)
def test_broadcast_exact(case, F):
    lens = _lens(case, F)
    seg, off = _seg(lens)
    nb = len(lens)
    v = th.randn(nb, F, device=DEV)
    sid = th.from_numpy(_seg_ids(off)).to(DEV)
    out, = _twice(lambda: (B.segment_broadcast(seg, v),))
    assert th.equal(out, v[sid])
    assert th.equal(out, v[th.repeat_interleave(th.tensor(lens, dtype=th.int64, device=DEV))]
                    if nb else out)


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("case", CASES)
def test_float_sums_within_the_summation_bound(case, F):
    lens = _lens(case, F)
    seg, off = _seg(lens)
    n, nb = int(off[-1]), len(lens)
    x, w, v = th.randn(n, F), th.randn(n), th.randn(nb, F)
    cnt = np.diff(off).astype(np.float64)

    def run():
        xt, wt = x.to(DEV), w.to(DEV)
        return (B.segment_reduce("sum", seg, xt), B.segment_reduce("mean", seg, xt),
                B.segment_reduce("sum", seg, xt, wt), B.segment_rowdot(seg, xt, v.to(DEV)))

    s, m, ws, rd = (t.cpu().numpy().astype(np.float64) for t in _twice(run))
    x64, w64, v64 = x.numpy().astype(np.float64), w.numpy().astype(np.float64), v.numpy().astype(np.float64)
    nn = cnt[:, None]

    def check(got, ref, mag, terms, what):
        err, bound = np.abs(got - ref), 1.01 * (terms + 2) * U * mag
        print(what, "max err / bound", float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0)
        assert (err <= bound).all(), what

    check(s, _per_segment(lambda r: r.sum(0), x64, off, 0.0),
          _per_segment(lambda r: np.abs(r).sum(0), x64, off, 0.0), nn, "sum")
    check(m, _per_segment(lambda r: r.mean(0), x64, off, 0.0),
          _per_segment(lambda r: np.abs(r).sum(0), x64, off, 0.0) / np.maximum(nn, 1), nn, "mean")
    wx = x64 * w64[:, None]
    check(ws, _per_segment(lambda r: r.sum(0), wx, off, 0.0),
          _per_segment(lambda r: np.abs(r).sum(0), wx, off, 0.0), nn, "weighted sum")
    sid = _seg_ids(off)
    check(rd, (x64 * v64[sid]).sum(1), np.abs(x64 * v64[sid]).sum(1), F, "rowdot")


def _softmax_ref(s64, off):
    out = np.empty_like(s64)
    for b in range(len(off) - 1):
        r = s64[off[b]:off[b + 1]]
        if len(r):
            e = np.exp(r - r.max(0))
            out[off[b]:off[b + 1]] = e / e.sum(0)
    return out


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("case", CASES)
def test_softmax_forward_backward(case, F):
    lens = _lens(case, F)
    seg, off = _seg(lens)
    n = int(off[-1])
    s, ga = th.randn(n, F) * 3, th.randn(n, F)

    def run():
        st = s.to(DEV).requires_grad_()
        a = B.segment_softmax(seg, st)
        g, = th.autograd.grad(a, st, ga.to(DEV))
        return a.detach(), g

    a, g = _twice(run)
    assert a.shape == (n, F)  # nothing for an empty segment: only rows have outputs
    ref = _softmax_ref(s.numpy().astype(np.float64), off)
    assert np.allclose(a.cpu().numpy().astype(np.float64), ref, rtol=1e-5, atol=1e-7)
    # every segment's column sums to 1 within n 2^-23
    a64 = a.cpu().numpy().astype(np.float64)
    for b in range(len(lens)):
        if lens[b]:
            assert (np.abs(a64[off[b]:off[b + 1]].sum(0) - 1.0) <= lens[b] * 2.0 ** -23).all()
    # a ga - a sum(a ga), float64 from the fp32 forward output (softmax.py:103-112)
    g64 = ga.numpy().astype(np.float64)
    S = _per_segment(lambda r: r.sum(0), a64 * g64, off, 0.0)
    gref = a64 * g64 - a64 * S[_seg_ids(off)]
    assert np.allclose(g.cpu().numpy().astype(np.float64), gref, rtol=1e-4, atol=1e-6)


def test_softmax_of_all_minus_inf_is_nan():
    R = K.segment_chunk_rows(2)
    lens = [3, R + 5, 4]
    seg, off = _seg(lens)
    s = th.randn(int(off[-1]), 2)
    s[off[1]:off[2], 0] = -float("inf")
    a = B.segment_softmax(seg, s.to(DEV)).cpu()
    assert th.isnan(a[off[1]:off[2], 0]).all()
    keep = th.ones_like(s, dtype=th.bool)
    keep[off[1]:off[2], 0] = False
    ref = th.from_numpy(_softmax_ref(s.numpy().astype(np.float64), off))
    assert th.allclose(a[keep].double(), ref[keep], rtol=1e-5, atol=1e-7)


def test_backward_takes_gradients_that_are_offset_views():
    """th.cat hands each input a slice of the joint gradient: after 3 floats, a contiguous
    view 12 bytes into its buffer.  The backward of rowdot and of a scaled broadcast pass
    such a gradient to the reduce as its per-row scalars."""
    lens = [5, 0, 70, 2]
    seg, off = _seg(lens)
    n = int(off[-1])
    x, v, s = _t(_ints(np.random.default_rng(1), (n, 8), -8, 8)), th.randn(4, 8, device=DEV), \
        th.randn(n, device=DEV)
    gy = th.randn(3 + n, device=DEV)
    res = []
    for joined in (True, False):
        xt, vt, st = x.clone().requires_grad_(), v.clone().requires_grad_(), s.clone().requires_grad_()
        rd = B.segment_rowdot(seg, xt, vt) + B.segment_broadcast(seg, vt, st).sum(1)
        if joined:
            pad = th.zeros(3, device=DEV, requires_grad=True)
            res.append(th.autograd.grad(th.cat([pad, rd]), (xt, vt, st), gy))
        else:
            res.append(th.autograd.grad(rd, (xt, vt, st), gy[3:].clone()))
    for a, b in zip(*res):
        assert th.equal(a, b)


# ---- the readout functions on a dgl.batch of GPU graphs ---------------------------------------
def _gpu_graphs(sizes, F):
    gs = []
    for i, (n, m) in enumerate(sizes):
        g = dgl.DGLGraph()
        g.add_nodes(n)
        rng = np.random.default_rng(i)
        if m:
            g.add_edges(rng.integers(0, n, m), rng.integers(0, n, m))
        g.ndata["h"] = th.randn(n, F, device=DEV)
        g.ndata["w"] = th.randn(n, 1, device=DEV)
        g.edata["h"] = th.randn(m, F, device=DEV)
        g.edata["w"] = th.rand(m, 1, device=DEV) + 0.5
        gs.append(g)
    return gs


def _close(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert th.allclose(a, b, rtol=1e-5, atol=1e-6, equal_nan=True), (a - b).abs().max()


@pytest.mark.parametrize("kind", ["nodes", "edges"])
def test_readout_functions_match_per_graph_torch(kind):
    F = 6
    gs = _gpu_graphs([(5, 7), (1, 0), (0, 0), (300, 1000), (4, 3)], F)
    bg = dgl.batch(gs)
    assert bg.batch_size == 5
    parts = dgl.unbatch(bg)
    frame = (lambda g: g.ndata) if kind == "nodes" else (lambda g: g.edata)
    fn = lambda name: getattr(dgl, "%s_%s" % (name, kind))
    x = [frame(g)["h"] for g in parts]
    w = [frame(g)["w"] for g in parts]
    zero = th.zeros(F, device=DEV)
    _close(fn("sum")(bg, "h"), th.stack([t.sum(0) for t in x]))
    _close(fn("sum")(bg, "h", "w"), th.stack([(t * u).sum(0) for t, u in zip(x, w)]))
    _close(fn("mean")(bg, "h"), th.stack([t.mean(0) if len(t) else zero for t in x]))
    if kind == "edges":  # positive weights: the weighted mean is well conditioned
        ref = th.stack([(t * u).sum(0) / u.sum() for t, u in zip(x, w)])
        _close(fn("mean")(bg, "h", "w"), ref)  # 0 / 0 = nan for graphs without edges, as the reference
    _close(fn("max")(bg, "h"), th.stack([t.max(0)[0] if len(t) else zero - float("inf") for t in x]))
    _close(fn("softmax")(bg, "h"), th.cat([th.softmax(t, 0) for t in x]))
    v = th.randn(5, 3, device=DEV)
    assert th.equal(fn("broadcast")(bg, v), th.cat([v[i:i + 1].expand(len(t), 3) for i, t in enumerate(x)]))
    k = 3
    for desc in (True, False):
        vals, idx = fn("topk")(bg, "h", k, descending=desc, idx=-1)
        assert vals.shape == (5, k, F) and idx.shape == (5, k)
        for i, t in enumerate(x):
            order = th.argsort(t[:, -1], descending=desc)[:k]
            ref = th.zeros(k, F, device=DEV)
            ref[:len(order)] = t[order]
            assert th.equal(vals[i], ref)  # zero rows past the graph's size (readout.py:502-507)
            assert th.equal(idx[i, :len(order)], order)
        vals, idx = fn("topk")(bg, "h", k, descending=desc)
        assert vals.shape == (5, k, F) and idx.shape == (5, k, F)
        for i, t in enumerate(x):
            ref = th.zeros(k, F, device=DEV)
            srt = th.sort(t, 0, descending=desc)[0][:k]
            ref[:len(srt)] = srt
            assert th.equal(vals[i], ref)


def test_topk_pads_graphs_smaller_than_k():
    gs = _gpu_graphs([(2, 1), (6, 4)], 3)
    bg = dgl.batch(gs)
    vals, _ = dgl.topk_nodes(bg, "h", 4, idx=0)
    assert vals.shape == (2, 4, 3)
    assert th.equal(vals[0, 2:], th.zeros(2, 3, device=DEV))
    h0 = gs[0].ndata["h"]
    assert th.equal(vals[0, :2], h0[th.argsort(h0[:, 0], descending=True)])


def test_unbatched_graph_reads_out_as_a_batch_of_one():
    g = _gpu_graphs([(9, 5)], 4)[0]
    _close(dgl.sum_nodes(g, "h"), g.ndata["h"].sum(0, keepdim=True))
    _close(dgl.max_edges(g, "h"), g.edata["h"].max(0, keepdim=True)[0])


def test_errors():
    bg = dgl.batch(_gpu_graphs([(3, 2), (4, 1)], 4))
    seg = dgl.readout.segments(bg, "nodes", DEV)
    with pytest.raises(dgl.DGLError, match="first dimension 7"):
        B.segment_reduce("sum", seg, th.zeros(6, 4, device=DEV))
    out = th.empty(2, 4, device=DEV)
    with pytest.raises(dgl.DGLError, match="rows"):  # the library's own shape check
        K.segment_reduce("sum", seg, th.zeros(6, 4, device=DEV), None, out)
    with pytest.raises(dgl.DGLError, match="contiguous"):
        K.segment_reduce("sum", seg, th.zeros(4, 7, device=DEV).t(), None, out)
    with pytest.raises(dgl.DGLError, match="float32"):
        K.segment_reduce("sum", seg, th.zeros(7, 4, device=DEV, dtype=th.float64), None, out)
    with pytest.raises(dgl.DGLError, match="feature size"):
        K.segment_reduce("sum", seg, th.zeros(7, 4, device=DEV), None, th.empty(2, 5, device=DEV))
    with pytest.raises(dgl.DGLError, match="arg goes with max"):
        K.segment_reduce("max", seg, th.zeros(7, 4, device=DEV), None, out)
    # the readout functions take what the frames hold: a non-contiguous column is copied
    bg.ndata["t"] = th.randn(4, 7, device=DEV).t()
    _close(dgl.sum_nodes(bg, "t"), th.stack([bg.ndata["t"][:3].sum(0), bg.ndata["t"][3:].sum(0)]))
