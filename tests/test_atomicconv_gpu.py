"""AtomicConv on csrc/kernels_atomic.hip (k_atomic_aggregate, k_atomic_edge_grad, k_atomic_fixup,
k_atomic_param_reduce) and CFConv on the builtins, against ONE fp64 restatement of the
reference's formula (_reference: the radial filters, a product per edge, index_add, in plain
torch); gradients by autograd on it.

Graph: rows laid from position 0 of the in-CSR with 63, 1, 65, 0, 64 and 80 * 64 edges (one
short of a chunk boundary, ending on it, starting on it, empty, straddling, a hub with three
fixup segments), two trailing empty rows, edge ids a random permutation of the positions
(distances indexed by position fail); "bip" is the same table through dgl.bipartite with
N_src != N_dst.

Exact cases: gamma = 10^4, r in {0, 1, 2, 3}, c in {2^100, 0.5}, d in {0, 1, 2, 3}: e_k(d) is
exactly [d == r_k and d <= c_k] in fp32 and fp64 (exp(-10^4 n^2) is 0, cos(pi d / 2^100) is 1),
x is integer-valued in [-3, 3] and the absolute mass is below 2^24 (asserted), so every
order of addition is exact and the kernel must th.equal the fp64 sums; every gradient is
then exactly zero (its terms carry d - r = 0, sin(0) or factors below fp32's range).

Tolerance cases: per element |got - ref| <= c 2^-24 S with c = depth + T + 56 and S the fp64
sum of |x| |g| h_k and the derivative factors with f_k replaced by its bound 1 (DESIGN.md
4.7d has the derivation; nothing in it is measured)."""
import functools
import math
import types

import numpy as np
import pytest
import torch as th

import dgl
from dgl import backend as B, kernel as K
from dgl.nn.pytorch import AtomicConv, CFConv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD, SENT, U = 16, -12345.5, 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _graph(kind):
    CH = K.ATOMIC_CHUNK
    rows = [CH - 1, 1, CH + 1, 0, CH, 80 * CH]
    rng = np.random.default_rng(7)
    dst = np.repeat(np.arange(len(rows)), rows)
    n_dst = len(rows) + 2                       # two more rows without edges
    n_src = n_dst if kind == "homo" else n_dst + 5
    src = rng.integers(0, n_src, len(dst))
    perm = rng.permutation(len(dst))
    G = types.SimpleNamespace(n_src=n_src, n_dst=n_dst, E=len(dst))
    if kind == "homo":
        G.g = dgl.DGLGraph()
        G.g.add_nodes(n_dst)
        G.g.add_edges(src[perm], dst[perm])
    else:
        G.g = dgl.bipartite((src[perm], dst[perm]), num_nodes=(n_src, n_dst))
    G.s, G.d = th.from_numpy(src[perm]).to(DEV), th.from_numpy(dst[perm]).to(DEV)
    G.deg_in = th.bincount(G.d, minlength=n_dst).double()
    G.gidx = G.g._graph.get_immutable_gidx(th.device(DEV))
    return G


def _reference(G, x, d, c, r, gam, go=None):
    """out (N_dst, T K) of the reference's formula in the dtype of its arguments (c, r, gam
    flat); with go also S, the terms' absolute values with f_k replaced by [d <= c_k]."""
    T, nk = x.shape[1], c.shape[0]
    dd = d.reshape(-1, 1)
    t = dd - r
    h = th.exp(-gam * t * t)
    m = dd <= c
    e = h * th.where(m, 0.5 * (th.cos(math.pi * dd / c) + 1), th.zeros_like(h))

    def agg(xs, w):
        msg = xs[G.s][:, :, None] * w[:, None, :]
        return msg.new_zeros(G.n_dst, T, nk).index_add(0, G.d, msg).flatten(1)
    if go is None:
        return agg(x, e)
    with th.no_grad():
        hm = h * m
        D = th.einsum("et,etk->ek", x[G.s].abs(), go.abs().view(-1, T, nk)[G.d])
        S = {"out": agg(x.abs(), hm), "scaling": (D * hm * t * t).sum(0),
             "means": (D * hm * 2 * gam * t.abs()).sum(0),
             "cutoffs": (D * hm * 0.5 * math.pi * dd / c ** 2).sum(0),
             "dist": (D * hm * (2 * gam * t.abs() + 0.5 * math.pi / c)).sum(1)}
    return agg(x, e), S


# every TT instance (T = 1, 2, 3, 8, 9, 17 and 32 -> 1, 2, 4, 8, 16, 32), every group count
# (K = 1, 2, 3, 5 and 8, 12, 32, 33 and 64 -> G = 64, 32, 16, 8, 4, 2, 1), two and four K tiles
@pytest.mark.parametrize("kind", ["homo", "bip"])
@pytest.mark.parametrize("nk,T", [(1, 1), (5, 8), (8, 3), (32, 17), (33, 32), (64, 1), (65, 8),
                                  (200, 3), (5, 32), (12, 2), (3, 9), (2, 17)])
def test_atomic_kernels_exact(kind, nk, T):
    G = _graph(kind)
    gen = th.Generator(device=DEV).manual_seed(nk * 100 + T)

    def padded(vals, n, m):   # NaN rows behind
        buf = th.full((n + PAD, m), float("nan"), device=DEV)
        buf[:n] = vals
        return buf[:n]
    x = padded(th.randint(-3, 4, (G.n_src, T), device=DEV, generator=gen).float(), G.n_src, T)
    d = padded(th.randint(0, 4, (G.E, 1), device=DEV, generator=gen).float(), G.E, 1)
    g = padded(th.randint(-3, 4, (G.n_dst, T * nk), device=DEV, generator=gen).float(), G.n_dst, T * nk)
    ks = th.arange(nk, device=DEV)
    r, gam = (ks % 4).float(), th.full((nk,), 1e4, device=DEV)
    c = th.where(ks % 3 == 0, th.tensor(0.5, device=DEV), th.tensor(2.0 ** 100, device=DEV))
    par = [p.double().requires_grad_() for p in (d, c, r, gam)]
    want = _reference(G, x.double(), *par)
    mass = _reference(G, x.double().abs(), *[p.detach() for p in par])
    assert float(mass.max()) * 2 < 2 ** 24
    want_grads = th.autograd.grad(want, par, g.double())
    out = th.full((G.n_dst + PAD, T * nk), SENT, device=DEV)
    K.atomic_aggregate(G.gidx, x, d, c, r, gam, out[:G.n_dst])
    assert th.equal(out[:G.n_dst], want.detach().float()) and bool((out[G.n_dst:] == SENT).all())
    for asked in ((True, True, True, True), (True, False, False, False), (False, True, False, True)):
        bufs = [th.full((n + PAD,), SENT, device=DEV) for n in (G.E, nk, nk, nk)]
        K.atomic_edge_grad(G.gidx, x, g, d, c, r, gam,
                           *[b[:n] if a else None for b, n, a in zip(bufs, (G.E, nk, nk, nk), asked)])
        for b, n, a, w in zip(bufs, (G.E, nk, nk, nk), asked, want_grads):
            assert th.equal(b[:n], w.reshape(-1).float()) if a else bool((b[:n] == SENT).all())
            assert bool((b[n:] == SENT).all())


def _case(nk, types, graph=None, seed=0):
    """(conv, graph, feat, distances, grad_out, fp64 reference values, bounds) of a module case."""
    G = _graph("homo")
    gen = th.Generator(device=DEV).manual_seed(seed + nk)
    use = None if types is None else th.arange(1, types + 1).float()
    T = 1 if types is None else types
    conv = AtomicConv(th.linspace(1.5, 4.0, nk), th.linspace(0.0, 4.0, nk),
                      th.rand(nk) * 0.25 + 0.2, use).to(DEV)
    rp = conv.radial_pooling
    if types is None:
        feat = th.randn(G.n_src, 1, device=DEV, generator=gen)
    else:
        feat = th.randint(1, types + 1, (G.n_src, 1), device=DEV, generator=gen).float()
    dist = th.rand(G.E, 1, device=DEV, generator=gen) * 3.9 + 0.1
    with th.no_grad():   # distances equal to, one float below and one above c_0 and c_last
        cs = rp.interaction_cutoffs.view(-1)[[0, -1]].repeat_interleave(3)
        dist[:6, 0] = th.stack([cs[0], th.nextafter(cs[1], cs[1] - 1), th.nextafter(cs[2], cs[2] + 1),
                                cs[3], th.nextafter(cs[4], cs[4] - 1), th.nextafter(cs[5], cs[5] + 1)])
    go = th.randn(G.n_dst, T * nk, device=DEV, generator=gen)
    x = feat if types is None else (feat == conv.features_to_use).float()
    par = [p.detach().double().reshape(-1).requires_grad_() for p in
           (dist, rp.interaction_cutoffs, rp.rbf_kernel_means, rp.rbf_kernel_scaling)]
    # the bound's input condition: no filter value below exp(-8), distances not negative
    with th.no_grad():
        assert float((par[3] * (par[0].view(-1, 1) - par[2]) ** 2).max()) <= 8 and float(dist.min()) >= 0
    want, S = _reference(G, x.double(), *par, go=go.double())
    ref = dict(zip(("dist", "cutoffs", "means", "scaling"), th.autograd.grad(want, par, go.double())),
               out=want.detach())
    depth = {"out": G.deg_in.view(-1, 1), "dist": nk, "cutoffs": G.E, "means": G.E, "scaling": G.E}
    return conv, graph or G.g, feat, dist, go, ref, {k: (depth[k] + T + 56) * U * S[k] for k in S}


def _run(conv, g, feat, dist, go):
    conv.zero_grad()
    dl = dist.detach().requires_grad_()
    out = conv(g, feat, dl)
    out.backward(go)
    rp = conv.radial_pooling
    return {"out": out.detach(), "dist": dl.grad, "cutoffs": rp.interaction_cutoffs.grad,
            "means": rp.rbf_kernel_means.grad, "scaling": rp.rbf_kernel_scaling.grad}


def _check(got, ref, bound, what):
    for k, b in bound.items():
        err = (got[k].double().reshape(ref[k].shape) - ref[k]).abs()
        print(what, k, "max err / bound: %.3g" % float((err / b.clamp(min=1e-300)).max()))
        assert bool((err <= b).all()), (what, k)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("nk", [5, 70])
@pytest.mark.parametrize("types", [None, 8])
def test_atomicconv_forward_backward(types, nk, fused):
    conv, g, feat, dist, go, ref, bound = _case(nk, types)
    conv.fused = fused
    x = feat if types is None else (feat == conv.features_to_use).float()
    assert (conv._route(g, x, dist) is not None) == fused
    _check(_run(conv, g, feat, dist, go), ref, bound, "fused" if fused else "unfused")


@pytest.mark.parametrize("what", ["K257", "T33", "feat_grad", "bits64"])
def test_atomicconv_fallbacks(what):
    """Shapes just outside atomic_ok, a feat that requires grad and a 64-bit graph: the
    reference's own steps, held to the same bound."""
    g64 = dgl.DGLGraph(_graph("homo").g._graph.asbits(64)) if what == "bits64" else None
    conv, g, feat, dist, go, ref, bound = _case(257 if what == "K257" else 5,
                                                33 if what == "T33" else None, graph=g64)
    if what == "feat_grad":
        feat.requires_grad_()
    x = feat if conv.features_to_use is None else (feat == conv.features_to_use).float()
    assert B.atomic_route(g, x, dist, conv.radial_pooling.interaction_cutoffs.numel()) is None
    _check(_run(conv, g, feat, dist, go), ref, bound, what)


def test_atomicconv_reproducible_on_the_hub():
    conv, g, feat, dist, go, _, _ = _case(12, 8, seed=5)
    a, b = _run(conv, g, feat, dist, go), _run(conv, g, feat, dist, go)
    assert all(th.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("hidden", [6, 70])
def test_cfconv_forward_backward(hidden):
    """project_node / project_edge, u_mul_e + sum on the builtins, project_out against the same
    steps in fp64, within the conv-zoo tests' tolerance for the builtins."""
    G = _graph("homo")
    th.manual_seed(hidden)
    conv = CFConv(5, 3, hidden, 4).to(DEV)
    ref = CFConv(5, 3, hidden, 4).to(DEV).double()
    ref.load_state_dict(conv.state_dict())
    nf, ef = th.randn(G.n_src, 5, device=DEV), th.randn(G.E, 3, device=DEV)
    go = th.randn(G.n_dst, 4, device=DEV)
    leaves = [t.clone().requires_grad_() for t in (nf, ef)]
    out = conv(G.g, *leaves)
    out.backward(go)
    l64 = [t.double().requires_grad_() for t in (nf, ef)]
    msg = ref.project_node(l64[0])[G.s] * ref.project_edge(l64[1])
    want = ref.project_out(msg.new_zeros(G.n_dst, hidden).index_add(0, G.d, msg))
    want.backward(go.double())
    pairs = [(out, want)] + [(a.grad, b.grad) for a, b in zip(leaves, l64)]
    pairs += [(p.grad, q.grad) for p, q in zip(conv.parameters(), ref.parameters())]
    for a, b in pairs:
        assert th.allclose(a.double(), b, rtol=1e-4, atol=1e-4), (a.double() - b).abs().max()
