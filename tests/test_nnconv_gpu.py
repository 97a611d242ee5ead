"""NNConv on csrc/kernels_nnconv.hip (k_nnconv_aggregate, k_nnconv_backward, k_nnconv_fixup)
against ONE fp64 restatement of the reference's formula (_reference: per-edge matrices, a
product per edge, index_add, in plain torch); gradients by autograd on it.

Graph, per chunk length CH = K.nnconv_chunk(in, out, nnz): a per-row table laid from
position 0 of the in-CSR so that chunk boundaries fall where the comments say, one hub of
80 CH edges (three fixup segments), 70 CH of all edges from source 0 (three segments in the
out-CSR too, the other sources random, some without edges), edge ids a random permutation
of the positions (W indexed by position fails); "bip" is the same table through
dgl.bipartite with N_src != N_dst.  These tables are small, so the chunk rule's "fewer than
4,096 chunks" branch picks CH; "big" appends rows of 19 edges until the rule's other branch
holds (64 -> 64 at CH = 4, the MPNN setting: 16,384 edges, 268 MB of W -- the fewest edges
at which the library picks that chunk length for that shape).

Exact cases: x, W and g are integer-valued in [-3, 3], the row scale in {0, 1, 2}, the
absolute mass is below 2^24 (asserted: a condition on the inputs) and the build has
-ffp-contract=off, so every partial sum is exact in any order and the kernels must
th.equal the fp64 sums.

Tolerance cases: per element |got - ref| <= c 2^-24 S, S the fp64 value of the same formula
on absolute values, c = the depth of the element's addition tree in the code that runs (the
kernels' own for the fused form, the builtins' for the fallbacks: _depths) plus the GEMMs on
its path plus single roundings (DESIGN.md 4.7c has the derivation)."""
import functools
import types

import numpy as np
import pytest
import torch as th

import dgl
from dgl import kernel as K
from dgl.nn.pytorch import NNConv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD, SENT, LIMIT, U, FE = 16, -12345.5, float(2 ** 24), 2.0 ** -24, 5


@functools.lru_cache(maxsize=None)
def _graph(kind, fin, fout, big=False):
    # 0: a width the kernels do not serve; big: the chunk length of a graph of many edges
    CH = K.nnconv_chunk(fin, fout, 1 << 40 if big else 1) or 64
    rows = [CH - 1,   # ends one short of the first boundary
            1,        # one edge; ends exactly on the boundary
            CH + 1,   # starts on a boundary, one edge into the next chunk
            0,        # no in-edge
            CH,       # starts one past a boundary: straddles the next
            80 * CH]  # hub: 3 fixup segments of continuation chunks
    if big:
        rows += [19] * ((4096 * CH - sum(rows)) // 19 + 1)
    rng = np.random.default_rng(7)
    dst = np.repeat(np.arange(len(rows)), rows)
    n_dst = len(rows) + 2                       # two more rows without edges
    n_src = n_dst if kind == "homo" else n_dst + 5
    src = rng.integers(1, n_src, len(dst))
    src[rng.permutation(len(dst))[:70 * CH]] = 0
    perm = rng.permutation(len(dst))
    G = types.SimpleNamespace(n_src=n_src, n_dst=n_dst, E=len(dst), CH=CH)
    if kind == "homo":
        G.g = dgl.DGLGraph()
        G.g.add_nodes(n_dst)
        G.g.add_edges(src[perm], dst[perm])
    else:
        G.g = dgl.bipartite((src[perm], dst[perm]), num_nodes=(n_src, n_dst))
    G.s, G.d = th.from_numpy(src[perm]).to(DEV), th.from_numpy(dst[perm]).to(DEV)
    G.deg_in = th.bincount(G.d, minlength=n_dst).double()
    G.deg_out = th.bincount(G.s, minlength=n_src).double()
    G.gidx = G.g._graph.get_immutable_gidx(th.device(DEV))
    assert K.nnconv_chunk(fin, fout, G.E) in (CH, 0)   # the rows lie around THIS call's chunks
    return G


def _reference(G, agg, xs, W):
    """The reference's aggregation in the dtype of its arguments: u_mul_e of (N, in, 1) with
    W (E, in, out), the reducer, the sum over `in`."""
    if agg == "max":
        msg = xs[G.s][:, :, None] * W
        red = msg.new_full((G.n_dst,) + tuple(msg.shape[1:]), -float("inf"))
        red = red.index_reduce(0, G.d, msg, "amax")
        return th.where(th.isinf(red), th.zeros_like(red), red).sum(1)
    msg = th.einsum("ei,eio->eo", xs[G.s], W)
    rst = msg.new_zeros(G.n_dst, msg.shape[1]).index_add(0, G.d, msg)
    return rst / G.deg_in.clamp(min=1).view(-1, 1) if agg == "mean" else rst


# ---- exact ------------------------------------------------------------------------------
# every instance once: the vector ones (out = 4 .. 256), the scalar ones (1, 2 and 4 columns
# per lane), `in` just past the dx accumulator tile (32 row steps: 129 at out = 64, 33 at
# out = 256 and in the scalar instances), chunk lengths 1, 2, 4, 16, 32, 64, and 64 -> 64 at
# the chunk length of a large graph
@pytest.mark.parametrize("kind,fin,fout,big", [
    (kind, fin, fout, False) for fin, fout in [
        (1, 1), (3, 4), (5, 64), (64, 64), (7, 5), (33, 68), (2, 256), (3, 8), (9, 16), (5, 32),
        (3, 128), (2, 132), (129, 64), (33, 256), (256, 3)] for kind in ("homo", "bip")
] + [("homo", 64, 64, True)])
def test_nnconv_kernels_exact(kind, fin, fout, big):
    G = _graph(kind, fin, fout, big)
    assert not big or G.CH == 4
    gen = th.Generator(device=DEV).manual_seed(fin * 1000 + fout)

    def ints(n, m, pad=PAD):   # integer-valued in [-3, 3], NaN rows behind
        buf = th.full((n + pad, m), float("nan"), device=DEV)
        buf[:n] = th.randint(-3, 4, (n, m), device=DEV, generator=gen).float()
        return buf[:n]
    x, w, g = ints(G.n_src, fin), ints(G.E, fin * fout, pad=1), ints(G.n_dst, fout)
    scale = th.randint(0, 3, (G.n_dst,), device=DEV, generator=gen).float()   # 0, 1, 2: exact
    for sc in (None, scale):
        scd = 1.0 if sc is None else sc.double().view(-1, 1)
        want = []
        for f in (lambda t: t, th.abs):   # the values, then their absolute mass
            lx, lw = f(x.double()).requires_grad_(), f(w.double()).requires_grad_()
            out = _reference(G, "sum", lx, lw.view(G.E, fin, fout)) * scd
            want.append((out.detach(),) + th.autograd.grad(out, [lx, lw], f(g.double())))
        (want_out, want_dx, want_dw), mass = want
        assert max(float(m.max()) for m in mass) * 2 < LIMIT
        out = th.full((G.n_dst + PAD, fout), SENT, device=DEV)
        K.nnconv_aggregate(G.gidx, x, w, out[:G.n_dst], row_scale=sc)
        assert th.equal(out[:G.n_dst], want_out.float()) and bool((out[G.n_dst:] == SENT).all())
        for need_dx, need_dw in ((True, False), (False, True), (True, True)):
            dx = th.full((G.n_src + PAD, fin), SENT, device=DEV)
            dw = th.full((G.E + 1, fin * fout), SENT, device=DEV)
            K.nnconv_backward(G.gidx, x, w, g, sc, dx=dx[:G.n_src] if need_dx else None,
                              dw=dw[:G.E] if need_dw else None)
            assert th.equal(dx[:G.n_src], want_dx.float()) if need_dx else bool((dx == SENT).all())
            assert th.equal(dw[:G.E], want_dw.float()) if need_dw else bool((dw == SENT).all())
            assert bool((dx[G.n_src:] == SENT).all()) and bool((dw[G.E:] == SENT).all())


# ---- tolerance --------------------------------------------------------------------------
def _depths(G, fin, fout, fused):
    """Additions on the longest path of out[v] and of dfeat[u].  Builtins:
    a sum over the row's edges per (in, out) element, then torch's sum over `in` (forward) or
    over the broadcast `out` (backward).  Kernels: a chunk's piece of a row in one lane
    (min(deg, CH) positions of ceil(in / RS) row steps; for dx one addition per position after
    a dot of NC columns), the cross-lane steps (log2 RS; log2 LR), then the fixup's fold over
    the row's at most ceil(deg / CH) continuation chunks, in segments of 32 beyond 32."""
    if not fused:
        return G.deg_in + fin, G.deg_out + fout
    lr = fout // 4
    vec = fout % 4 == 0 and 1 <= lr <= 64 and lr & (lr - 1) == 0
    LR, NC = (lr, 4) if vec else (64, 1 if fout <= 64 else 2 if fout <= 128 else 4)
    RS = 64 // LR

    def fold(deg):
        nc = th.ceil(deg / G.CH)
        return th.where(nc <= 32, nc, 32 + th.ceil(nc / 32))
    return (G.deg_in.clamp(max=G.CH) * -(-fin // RS) + np.log2(RS) + fold(G.deg_in),
            G.deg_out.clamp(max=G.CH) + NC + np.log2(LR) + fold(G.deg_out))


def _run(conv, G, xs, xd, ef, go, fused):
    conv.fused = fused
    conv.zero_grad()
    leaves = [t.detach().requires_grad_() for t in (xs, xd, ef)]
    out = conv(G.g, (leaves[0], leaves[1]), leaves[2])
    out.backward(go)
    got = {"out": out.detach(), "feat": leaves[0].grad, "efeat": leaves[2].grad,
           "lw": conv.edge_nn.weight.grad, "lb": conv.edge_nn.bias.grad}
    if conv.bias is not None:
        got.update(bias=conv.bias.grad, res=conv.res_fc.weight.grad)
    return got


def _case(kind, agg, fin, fout, opt, fused=True, seed=0):
    """(conv, graph, inputs, fp64 reference values, per-element bounds) of one module case."""
    G = _graph(kind, fin, fout)
    th.manual_seed(seed + fin * 10 + fout)
    fd = fin if kind == "homo" else fin + 2
    conv = NNConv((fin, fd), fout, th.nn.Linear(FE, fin * fout), agg, residual=opt, bias=opt).to(DEV)
    if opt:
        with th.no_grad():
            conv.bias.normal_()
    xs, xd = th.randn(G.n_src, fin, device=DEV), th.randn(G.n_dst, fd, device=DEV)
    ef, go = th.randn(G.E, FE, device=DEV), th.randn(G.n_dst, fout, device=DEV)
    par = [t.detach().double() for t in (xs, xd, ef, conv.edge_nn.weight, conv.edge_nn.bias)]
    par += [conv.res_fc.weight.detach().double() if opt else None,
            conv.bias.detach().double() if opt else None]
    names = ["feat", None, "efeat", "lw", "lb", "res", "bias"]
    ref, S = {}, {}
    for store, f in ((ref, lambda t: t), (S, th.abs)):   # S: every factor's absolute value
        lv = [None if t is None else f(t).requires_grad_() for t in par]
        out = _reference(G, "sum" if agg == "max" and store is S else agg, lv[0],
                         (lv[2] @ lv[3].t() + lv[4]).view(G.E, fin, fout))
        if opt:
            out = out + lv[1][:G.n_dst] @ lv[5].t() + lv[6]
        keep = [(n, t) for n, t in zip(names, lv) if n and t is not None]
        grads = th.autograd.grad(out, [t for _, t in keep], f(go.double()))
        store.update({"out": out.detach(), **{n: gr for (n, _), gr in zip(keep, grads)}})
    # the depth of the element's own sum, the GEMMs on its path in any order (edge_nn: FE + 1
    # terms, the residual: fd, defeat: in out, the parameter gradients: E or N_dst), single
    # roundings (products, the row scale, the additions of residual and bias): 6
    d_out, d_feat = _depths(G, fin, fout, fused)
    lin = FE + 1
    c = {"out": d_out.view(-1, 1) + lin + fd + 6, "feat": d_feat.view(-1, 1) + lin + 6,
         "efeat": fin * fout + 6, "lw": G.E + 6, "lb": G.E + 6, "res": G.n_dst + 6, "bias": G.n_dst + 6}
    return conv, G, (xs, xd, ef, go), ref, {k: c[k] * U * S[k] for k in S}


def _check(got, ref, bound, what):
    for k, b in bound.items():
        err = (got[k].double() - ref[k]).abs()
        print(what, k, "max err / bound: %.3g" % float((err / b.clamp(min=1e-300)).max()))
        assert bool((err <= b).all()), (what, k)


# the scalar instance, the vector one, and `in` past the dx tile in each
@pytest.mark.parametrize("kind,agg,opt,fin,fout", [
    ("homo", "sum", False, 10, 6), ("homo", "mean", True, 10, 6), ("bip", "sum", True, 10, 6),
    ("bip", "mean", False, 5, 16), ("homo", "sum", True, 5, 16), ("homo", "mean", False, 33, 68),
    ("bip", "sum", True, 33, 68), ("homo", "mean", True, 129, 64), ("bip", "sum", False, 129, 64)])
def test_nnconv_forward_backward(kind, agg, opt, fin, fout):
    conv, G, (xs, xd, ef, go), ref, bound = _case(kind, agg, fin, fout, opt)
    w = conv.edge_nn(ef).view(-1, fin * fout)
    assert conv._route(G.g, xs, w) is not None
    _check(_run(conv, G, xs, xd, ef, go, True), ref, bound, "fused")


@pytest.mark.parametrize("agg,fin,fout,fused", [("max", 10, 6, True), ("sum", 10, 6, False),
                                                ("mean", 10, 257, True), ("sum", 257, 3, True)])
def test_nnconv_fallbacks(agg, fin, fout, fused):
    """'max', fused = False and a width just outside nnconv_ok: the reference's step order
    on the builtins, forward and backward, held to the bound of that order's depth."""
    conv, G, (xs, xd, ef, go), ref, bound = _case("homo", agg, fin, fout, True, fused=False)
    conv.fused = fused
    assert conv._route(G.g, xs, conv.edge_nn(ef).view(-1, fin * fout)) is None
    assert not K.nnconv_ok(10, 257) and not K.nnconv_ok(257, 3) and K.nnconv_ok(256, 256)
    got = _run(conv, G, xs, xd, ef, go, fused)
    if agg == "max":
        # not linear: the terms of S are the sum's, a bound for the max too.  Rows without
        # in-edges keep the builtin max reducer's identity (the lowest float, as in the
        # reference), which the sum over `in` overflows: the forward is held on the rows
        # with edges; no gradient flows through the others.
        has = G.deg_in > 0
        got, ref, bound = ({**d, "out": d["out"][has]} for d in (got, ref, bound))
    _check(got, ref, bound, "fallback")


def test_nnconv_forward_has_no_edge_sized_temporary():
    """A condition: NNConv.forward on the fused route allocates N out floats (the carry
    workspace is the library's), never something of W's size (268 MB here)."""
    G = _graph("homo", 64, 64, True)
    x, w = th.randn(G.n_src, 64, device=DEV), th.randn(G.E, 64 * 64, device=DEV)
    conv = NNConv(64, 64, lambda efeat: w, "mean", bias=False)   # W precomputed: not counted
    assert conv._route(G.g, x, w) is not None
    with th.no_grad():
        conv(G.g, x, None)                        # warm: the device index's own tables
        th.cuda.synchronize()
        th.cuda.reset_peak_memory_stats()
        before = th.cuda.memory_allocated()
        conv(G.g, x, None)
        th.cuda.synchronize()
    assert th.cuda.max_memory_allocated() - before < w.numel() * 4 / 2


def test_nnconv_reproducible_on_the_hub():
    conv, G, (xs, xd, ef, go), _, _ = _case("bip", "mean", 64, 64, True, seed=5)
    a = _run(conv, G, xs, xd, ef, go, True)
    b = _run(conv, G, xs, xd, ef, go, True)
    assert all(th.equal(a[k], b[k]) for k in a)
