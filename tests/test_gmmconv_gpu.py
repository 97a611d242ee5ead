"""GMMConv on csrc/kernels_gmm.hip (k_gmm_aggregate, k_gmm_fixup, k_gmm_edge_grad,
k_gmm_param_reduce) against ONE fp64 restatement of the reference's formula: per-edge
weights, index_add_, .sum(1), in plain torch; gradients by autograd on it.

Graph: a per-row table laid from position 0 of the in-CSR so that chunk boundaries
(CH = K.GMM_CHUNK positions) fall where the comments say, one 5,000-edge hub, random
sources, edge ids a random permutation of the positions (pseudo indexed by position
fails); "bip" is the same table through dgl.bipartite with N_src != N_dst.

Exact cases: inv_sigma = 0 makes every w_k = exp(-0) = 1, x is integer-valued with
absolute mass below 2^24 (asserted: a condition on the inputs), the build has
-ffp-contract=off, so every partial sum is exact in any order and K.gmm_aggregate must
th.equal the fp64 sum for every k, both directions.

Tolerance cases: per element |got - ref| <= c 2^-24 S, S the fp64 sum of the absolute
values of the element's terms, c = _c(depth) below (DESIGN.md 4.7b has the derivation):
the depth of the element's addition tree (any order), the GEMMs and dots on its path,
the rounding of g amplified by |g| <= G_MAX (asserted), exp's 1 ulp, 12 single roundings."""
import functools

import numpy as np
import pytest
import torch as th

import dgl
from dgl import kernel as K
from dgl.nn.pytorch import GMMConv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD, SENT, LIMIT, U, G_MAX = 16, -12345.5, float(2 ** 24), 2.0 ** -24, 8.0
CH = K.GMM_CHUNK
ROWS = [CH - 1,   # ends one short of the first boundary
        1,        # one edge; ends exactly on the boundary
        CH + 1,   # starts on a boundary, one edge into the next chunk
        0,        # no in-edge
        CH,       # starts one past a boundary: straddles the next
        5000]     # hub: 79 chunks, 3 fixup segments


class _G:
    pass


@functools.lru_cache(maxsize=None)
def _graph(kind):
    rng = np.random.default_rng(7)
    dst = np.repeat(np.arange(len(ROWS)), ROWS)
    n_dst = len(ROWS) + 2                       # two more rows without edges
    n_src = n_dst if kind == "homo" else n_dst + 5
    src = rng.integers(0, n_src, len(dst))
    perm = rng.permutation(len(dst))
    G = _G()
    G.n_src, G.n_dst, G.E = n_src, n_dst, len(dst)
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
    return G


def _weights(pseudo, mu, sig):
    return th.exp((-0.5 * (pseudo[:, None, :] - mu[None]) ** 2 * sig[None] ** 2).sum(-1))  # (E, K)


def _reference(G, agg, xs, xd, pseudo, mu, sig, W, res_w, bias, w=None):
    """The reference's forward in the dtype of its arguments: fc, u_mul_e, reducer, sum(1)."""
    n_k = mu.shape[0]
    w = _weights(pseudo, mu, sig) if w is None else w
    msg = (xs @ W.t()).view(xs.shape[0], n_k, -1)[G.s] * w[:, :, None]
    if agg == "max":
        red = msg.new_full((G.n_dst,) + tuple(msg.shape[1:]), -float("inf"))
        red = red.index_reduce(0, G.d, msg, "amax")
        red = th.where(th.isinf(red), th.zeros_like(red), red)
    else:
        red = msg.new_zeros((G.n_dst,) + tuple(msg.shape[1:])).index_add(0, G.d, msg)
        if agg == "mean":
            red = red / G.deg_in.clamp(min=1).view(-1, 1, 1)
    rst = red.sum(1)
    if res_w is not None:
        rst = rst + xd[:G.n_dst] @ res_w.t()
    return rst if bias is None else rst + bias


# ---- exact ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,transposed", [("homo", False), ("homo", True), ("bip", False),
                                             ("bip", True)])
@pytest.mark.parametrize("width,n_k", [(1, 1), (63, 3), (64, 1), (65, 3), (130, 3),
                                       (65, K.gmm_k_tile(65) + 1), (130, K.gmm_k_tile(130) + 1)])
def test_gmm_aggregate_exact(kind, transposed, width, n_k):
    G = _graph(kind)
    rows, cols = (G.n_src, G.n_dst) if transposed else (G.n_dst, G.n_src)
    ri, ci = (G.s, G.d) if transposed else (G.d, G.s)
    gen = th.Generator(device=DEV).manual_seed(width * 100 + n_k)
    xbuf = th.full((cols + PAD, width), float("nan"), device=DEV)
    xbuf[:cols] = th.randint(-3, 4, (cols, width), device=DEV, generator=gen).float()
    x = xbuf[:cols]
    pseudo = th.randn(G.E, 2, device=DEV, generator=gen)
    mu = th.randn(n_k, 2, device=DEV, generator=gen)
    scale = th.randint(0, 3, (rows,), device=DEV, generator=gen).float()   # 0, 1, 2: exact
    ref = th.zeros(rows, width, dtype=th.float64, device=DEV).index_add(0, ri, x.double()[ci])
    mass = th.zeros(rows, width, dtype=th.float64, device=DEV).index_add(0, ri, x.double().abs()[ci])
    assert float(mass.max()) * 2 < LIMIT
    for sc in (None, scale):
        buf = th.full((rows + PAD, n_k * width), SENT, device=DEV)
        K.gmm_aggregate(G.gidx, x, pseudo, mu, th.zeros_like(mu), buf[:rows], row_scale=sc,
                        transposed=transposed)
        want = (ref if sc is None else ref * sc.double().view(-1, 1)).float()
        assert th.equal(buf[:rows].view(rows, n_k, width), want[:, None, :].expand(-1, n_k, -1))
        assert bool((buf[rows:] == SENT).all())


# ---- tolerance --------------------------------------------------------------------------
def _c(depth, n_k, fi, fo, fd, dim):
    return depth + n_k * max(fi, fo) + fi + fo + fd + G_MAX * (3 * dim + 2) + 2 + 12


def _run(conv, G, agg, xs, xd, pseudo, go, fused):
    conv.fused = fused
    conv.zero_grad()
    leaves = [t.detach().requires_grad_() for t in (xs, xd, pseudo)]
    out = conv(G.g, (leaves[0], leaves[1]), leaves[2])
    out.backward(go)
    got = {"out": out.detach(), "feat": leaves[0].grad, "pseudo": leaves[2].grad,
           "mu": conv.mu.grad, "inv_sigma": conv.inv_sigma.grad, "fc": conv.fc.weight.grad}
    if conv.bias is not None:
        got["bias"] = conv.bias.grad
    return got


def _case(kind, agg, n_k, dim, fi, fo, opt, seed=0):
    """(conv, inputs, fp64 reference values, per-element bounds) of one module case."""
    G = _graph(kind)
    th.manual_seed(seed + n_k * 10 + dim)
    fd = fi if kind == "homo" else fi + 2
    conv = GMMConv((fi, fd), fo, dim, n_k, agg, residual=opt, bias=opt).to(DEV)
    pseudo = th.rand(G.E, dim, device=DEV) * 2 - 1
    with th.no_grad():
        conv.mu.uniform_(-1, 1)
        # |pseudo - mu| <= 2, so |g| <= dim 4 sigma^2 / 2 <= G_MAX
        conv.inv_sigma.uniform_(0.2, 1).mul_((G_MAX / (2.0 * dim)) ** 0.5)
        if opt:
            conv.bias.normal_()
    xs, xd = th.randn(G.n_src, fi, device=DEV), th.randn(G.n_dst, fd, device=DEV)
    go = th.randn(G.n_dst, fo, device=DEV)
    res_w = conv.res_fc.weight if opt else None
    par = [t.detach().double() for t in (xs, xd, pseudo, conv.mu, conv.inv_sigma, conv.fc.weight)]
    par += [res_w.detach().double() if opt else None, conv.bias.detach().double() if opt else None]
    w = _weights(par[2], par[3], par[4])
    assert float(w.log().abs().max()) <= G_MAX      # the condition: no weight underflows
    ref, S = {}, {}
    for store, f in ((ref, lambda t: t), (S, th.abs)):   # S: every factor's absolute value
        lv = [None if t is None else f(t).requires_grad_() for t in par]
        # the weights do not depend on signs: S keeps w and differentiates the linear part
        out = _reference(G, "sum" if agg == "max" and store is S else agg, *lv,
                         w=None if store is ref else w)
        names = ["feat", None, "pseudo", "mu", "inv_sigma", "fc", None, "bias"]
        keep = [(n, t) for n, t in zip(names, lv) if n and t is not None and (store is ref or n in
                                                                             ("feat", "fc", "bias"))]
        grads = th.autograd.grad(out, [t for _, t in keep], f(go.double()))
        store.update({"out": out.detach(), **{n: gr for (n, _), gr in zip(keep, grads)}})
    if agg != "max":   # S of the mixture's gradients, term by term
        sc = 1.0 / G.deg_in.clamp(min=1) if agg == "mean" else th.ones_like(G.deg_in)
        dA = th.einsum("vo,koi->vki", go.double().abs() * sc.view(-1, 1),
                       par[5].abs().view(n_k, fo, fi))
        dg = (par[0].abs()[G.s][:, None, :] * dA[G.d]).sum(-1) * w           # (E, K)
        t = par[2][:, None, :] - par[3][None]
        S["pseudo"] = (dg[:, :, None] * t.abs() * par[4][None] ** 2).sum(1)
        S["mu"] = (dg[:, :, None] * t.abs() * par[4][None] ** 2).sum(0)
        S["inv_sigma"] = (dg[:, :, None] * t ** 2 * par[4][None].abs()).sum(0)
    depth = {"out": G.deg_in.view(-1, 1), "feat": G.deg_out.view(-1, 1), "pseudo": n_k,
             "mu": G.E, "inv_sigma": G.E, "fc": G.n_dst + float(G.deg_in.max()), "bias": G.n_dst}
    bound = {k: _c(depth[k], n_k, fi, fo, fd, dim) * U * S[k] for k in S}
    return conv, G, (xs, xd, pseudo, go), ref, bound


def _check(got, ref, bound, what):
    for k, b in bound.items():
        err = (got[k].double() - ref[k]).abs()
        print(what, k, "max err / bound: %.3g" % float((err / b.clamp(min=1e-300)).max().detach()))
        assert bool((err <= b).all()), (what, k)


@pytest.mark.parametrize("kind,agg,n_k,dim,opt,fi,fo", [
    ("homo", "sum", 1, 1, False, 10, 6), ("homo", "mean", 3, 2, True, 10, 6),
    ("homo", "sum", 25, 2, True, 10, 6), ("homo", "mean", 32, 8, False, 10, 6),
    ("bip", "sum", 3, 8, True, 10, 6), ("bip", "mean", 25, 1, False, 10, 6),
    # more than one column per lane: the walks' and the edge gradient's NV = 2, 4, 8
    # instances, K past their tiles (9 > 8 and 4), the input gradient 70 floats wide
    ("bip", "mean", 9, 2, False, 65, 6), ("homo", "sum", 9, 2, True, 130, 70),
    ("homo", "sum", 9, 1, False, 300, 6)])
def test_gmmconv_forward_backward(kind, agg, n_k, dim, opt, fi, fo):
    conv, G, (xs, xd, pseudo, go), ref, bound = _case(kind, agg, n_k, dim, fi, fo, opt)
    assert conv._route(G.g, xs, pseudo) is not None
    _check(_run(conv, G, agg, xs, xd, pseudo, go, True), ref, bound, "fused")


@pytest.mark.parametrize("agg,n_k,fo,fused", [("max", 3, 6, True), ("sum", 3, 6, False),
                                              ("mean", 33, 6, True), ("sum", 3, 513, True)])
def test_gmmconv_fallbacks(agg, n_k, fo, fused):
    """'max', fused = False, and K or the output width (the input gradient's rows) just
    outside gmm_ok: the reference's step order, forward and backward."""
    conv, G, (xs, xd, pseudo, go), ref, bound = _case("homo", agg, n_k, 2, 10, fo, True)
    conv.fused = fused
    assert conv._route(G.g, xs, pseudo) is None
    assert not K.gmm_ok(10, 33, 2) and not K.gmm_ok(513, 3, 2)
    got = _run(conv, G, agg, xs, xd, pseudo, go, fused)
    if agg == "max":
        # not linear: the terms of S are the sum's, a bound for the max too.  Rows without
        # in-edges keep the builtin max reducer's identity (the lowest float, as in the
        # reference), which the K-sum overflows: the forward is held on the rows with edges;
        # no gradient flows through the others.
        has = G.deg_in > 0
        got, ref, bound = ({"out": d["out"][has], "feat": d["feat"], "fc": d["fc"]}
                           for d in (got, ref, bound))
    _check(got, ref, bound, "fallback")


def test_gmmconv_fused_agrees_with_unfused():
    conv, G, (xs, xd, pseudo, go), ref, bound = _case("homo", "mean", 3, 2, 10, 6, True, seed=3)
    a = _run(conv, G, "mean", xs, xd, pseudo, go, True)
    b = _run(conv, G, "mean", xs, xd, pseudo, go, False)
    for k in bound:   # both within the bound of the fp64 value: within twice it of each other
        assert bool(((a[k].double() - b[k].double()).abs() <= 2 * bound[k]).all()), k


def test_gmmconv_reproducible_on_the_hub():
    conv, G, (xs, xd, pseudo, go), _, _ = _case("homo", "sum", 25, 2, 10, 6, True, seed=5)
    a = _run(conv, G, "sum", xs, xd, pseudo, go, True)
    b = _run(conv, G, "sum", xs, xd, pseudo, go, True)
    assert all(th.equal(a[k], b[k]) for k in ("out", "mu", "inv_sigma", "pseudo", "feat", "fc"))
