"""RelGraphConv's "bdd" regulariser on the segment kernels of csrc/kernels_rgcn_bdd.hip
(k_rgcn_bdd<., ., ., TRANSPOSED>, k_rgcn_bdd_fixup, k_rgcn_bdd_wgrad, k_rgcn_bdd_wreduce)
through the module and through the C entries.  EXACT, not close, by the method of
test_rgcn_shapes_gpu.py: integer-valued inputs (x in [-2, 2], W in {-1, 0, 1}, norm in
{1, 2}, grad_out / bias / addend in [-4, 4]); the build has -ffp-contract=off and the
kernels only multiply and add, so while the absolute mass of every sum stays below 2^24
(asserted first: a condition on the inputs, not a tolerance) every partial sum is exact in
any order and each result must th.equal the fp64 per-edge bmm + index_add restatement.
Inputs have NaN tail rows, the C entries' outputs sentinel tail rows.

Graphs come from a per-row table of (relation, count) segments, laid out from position 0
of the (destination, relation) walk so that chunk boundaries (K.RGCN_BDD_CHUNK positions)
fall where the comments say; the weight-gradient rows give relations 3 / 4 / 5 one
segment in WCH - 1 / WCH / WCH + 1 rows (WCH = K.RGCN_BDD_WGRAD_CHUNK) and relation 6 one
in 2 WCH + 88 rows (three chunks)."""
import functools

import numpy as np
import pytest
import torch as th

import dgl
import dgl.backend as B
from dgl import kernel as K
from dgl.nn.pytorch import RelGraphConv
from test_rgcn_gpu import typed_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD, SENT, LIMIT = 16, -12345.5, float(2 ** 24)
CH, WCH = K.RGCN_BDD_CHUNK, K.RGCN_BDD_WGRAD_CHUNK

EDGE_ROWS = [
    [(0, CH - 24), (1, 23)],          # length chunk - 1
    [(2, 1)],                         # one edge; its segment ends exactly on the boundary
    [(0, 30), (1, CH - 30), (2, 1)],  # chunk + 1 from a boundary: (1, .) ends on the next one
    [],                               # no in-edge
    [(1, CH)],                        # length chunk, one relation, straddles a boundary
    [(r, 1) for r in (0, 1, 2, 7, 8, 9)],   # every edge another relation
    [(0, 3)],                         # one repeated (u, v, r) triple (sources set below)
]
HUB = [[(0, 2000), (1, 1000), (2, 2000)]]   # 5 000 positions: 79 chunks, 3 fixup segments
WGRAD_ROWS = [[(3, 1)] * (i < WCH - 1) + [(4, 1)] * (i < WCH) + [(5, 1)] * (i < WCH + 1) + [(6, 2)]
              for i in range(2 * WCH + 88)]
GRAPHS = {  # name: (row table, relations); relations 10 .. 127 of "full" have no edge (the
    # module caps the bases at the relation count, so 100 bases need 100 relations)
    "full": (EDGE_ROWS + HUB + WGRAD_ROWS, 128),
    "edges": (EDGE_ROWS, 128),
    "one-rel": (EDGE_ROWS + HUB, 1),          # R = 1: every relation id folds to 0
    "tiny": ([[(40, 1), (3, 2)], [], [(17, 1)]], 50),   # R larger than E
}


class _G:
    pass


@functools.lru_cache(maxsize=None)
def _graph(name):
    table, R = GRAPHS[name]
    rng = np.random.default_rng(5)
    dst = np.asarray([v for v, segs in enumerate(table) for _, c in segs for _ in range(c)])
    et = np.asarray([r % R for segs in table for r, c in segs for _ in range(c)])
    n = max(len(table), 8) + 3
    src = rng.integers(0, n, len(dst))
    src[dst == 6] = 5
    perm = rng.permutation(len(dst))   # edge ids interleave rows and relations
    G = _G()
    G.n, G.R, G.src, G.dst, G.et = n, R, src[perm], dst[perm], et[perm]
    G.g = dgl.DGLGraph()
    G.g.add_nodes(n)
    G.g.add_edges(G.src, G.dst)
    G.s, G.d, G.t = (th.from_numpy(a).to(DEV) for a in (G.src, G.dst, G.et))
    return G


def _ints(gen, shape, lo, hi, pad=0):
    """Integer-valued fp32; pad: the head of a buffer with `pad` NaN tail rows."""
    buf = th.full((shape[0] + pad,) + tuple(shape[1:]), float("nan"), device=DEV)
    buf[:shape[0]] = th.randint(lo, hi + 1, shape, device=DEV, generator=gen).float()
    return buf[:shape[0]]


def _reference(G, fi, fo, nb, x, w, norm, bias, loop_w):
    """fp64: per edge msg = norm_e x[u] (B, 1, s_i) @ W[r] (B, s_i, s_o), summed by
    destination, + bias + x loop_w."""
    si, so = fi // nb, fo // nb
    msg = th.bmm(x[G.s].reshape(-1, 1, si), w[G.t].reshape(-1, si, so)).reshape(-1, fo)
    if norm is not None:
        msg = msg * norm.reshape(-1, 1)
    out = th.zeros(G.n, fo, dtype=th.float64, device=DEV).index_add(0, G.d, msg)
    if bias is not None:
        out = out + bias + x @ loop_w
    return out


def _exact(G, fi, fo, nb, x, w, norm, bias, loop_w, go):
    """(out, grad x, grad w, grad bias, grad loop_w) of the reference as fp32, after the
    mass bound on every one of those sums."""
    opt = bias is not None
    res = []
    for f in (th.abs, lambda t: t):
        leaves = [f(t.double()).requires_grad_() for t in (x, w) + ((bias, loop_w) if opt else ())]
        out = _reference(G, fi, fo, nb, leaves[0], leaves[1],
                         None if norm is None else norm.double(), *(leaves[2:] or (None, None)))
        res.append([out.detach()] + list(th.autograd.grad(out, leaves, f(go.double()))))
    assert all(float(t.max()) < LIMIT for t in res[0])
    return [t.float() for t in res[1]] + [None] * (0 if opt else 2)


CASES = [  # (in, out, bases), graph, norm, bias + self-loop
    ((20, 20, 4), "full", "rewritten", True),      # 5 x 5 blocks, width no multiple of 64
    ((16, 16, 16), "full", None, False),           # 1 x 1
    ((8, 16, 2), "full", "const", True),           # non-square
    ((16, 8, 2), "full", "const", False),
    ((21, 49, 7), "full", None, True),             # odd 3 x 7
    ((64, 64, 2), "full", "const", False),         # 32 x 32
    ((130, 130, 2), "full", "const", True),        # columns past one and two 64-lane passes
    ((500, 500, 100), "full", "const", True),      # the link-prediction layer
    ((1024, 1024, 64), "edges", "const", False),   # in * s_o = 16384, the route's cap
    ((20, 20, 1), "one-rel", "const", True),       # one 20 x 20 block
    ((24, 16, 8), "tiny", None, True),
]


@pytest.mark.parametrize("shape,graph,norm_kind,opt", CASES)
def test_bdd_forward_backward_exact(shape, graph, norm_kind, opt):
    (fi, fo, nb), G = shape, _graph(graph)
    assert K.rgcn_bdd_ok(fi, fo, nb) and nb <= G.R
    gen = th.Generator(device=DEV).manual_seed(fi * 1000 + fo)
    x = _ints(gen, (G.n, fi), -2, 2, PAD)
    go = _ints(gen, (G.n, fo), -4, 4, PAD)
    norm = None if norm_kind is None else _ints(gen, (len(G.src), 1), 1, 2)
    conv = RelGraphConv(fi, fo, G.R, "bdd", nb, bias=opt, self_loop=opt).to(DEV)
    with th.no_grad():
        conv.weight.copy_(_ints(gen, tuple(conv.weight.shape), -1, 1))
        if opt:
            conv.h_bias.copy_(_ints(gen, (fo,), -4, 4))
            conv.loop_weight.copy_(_ints(gen, (fi, fo), -1, 1))
    assert B.rgcn_bdd_route(G.g, x, (G.R, fi, fo, nb), norm, G.t) is not None
    for step in range(2 if norm_kind == "rewritten" else 1):
        if step:
            norm.copy_(3 - norm)   # in place: 1 <-> 2; the call must see the new values
        ref = _exact(G, fi, fo, nb, x, conv.weight.detach(), norm, conv.h_bias.detach() if opt else None,
                     conv.loop_weight.detach() if opt else None, go)
        xi = x.detach().requires_grad_()
        conv.zero_grad()
        out = conv(G.g, xi, G.t, norm)
        out.backward(go)
        got = [out.detach(), xi.grad, conv.weight.grad] + \
              ([conv.h_bias.grad, conv.loop_weight.grad] if opt else [None, None])
        for name, a, b in zip(("out", "grad x", "grad weight", "grad bias", "grad loop_weight"), got, ref):
            assert b is None or th.equal(a, b), (name, step)
    # the C entries into sentinel-tailed buffers: the aggregation alone (+ bias, addend)
    gidx, state, nf, _ = B.rgcn_bdd_route(G.g, x, (G.R, fi, fo, nb), norm, G.t)
    w = conv.weight.detach()
    bufs = [th.full((r + PAD, c), SENT, device=DEV) for r, c in ((G.n, fo), (G.n, fi), tuple(w.shape))]
    o, gx, gw = (b[:b.shape[0] - PAD] for b in bufs)
    add = _ints(gen, (G.n, fo), -4, 4) if opt else None
    K.rgcn_bdd_forward(gidx, state, x, w, nb, nf, o, bias=conv.h_bias.detach() if opt else None, addend=add)
    K.rgcn_bdd_backward(gidx, state, x, w, nb, nf, go, gx, gw)
    plain = _exact(G, fi, fo, nb, x, w, norm, None, None, go)
    if opt:
        assert float((add.abs() + conv.h_bias.detach().abs()).max()) + 0 < LIMIT / 2
        plain[0] = (plain[0].double() + conv.h_bias.detach().double() + add.double()).float()
    for name, a, b, buf in zip(("out", "grad x", "grad weight"), (o, gx, gw), plain, bufs):
        assert th.equal(a, b), name
        assert bool((buf[-PAD:] == SENT).all()), name


def _module_run(conv, g, x, et, norm, fused):
    conv.use_fused = fused
    conv.zero_grad()
    xi = x.detach().requires_grad_()
    out = conv(g, xi, et, norm)
    out.pow(2).sum().backward()
    return [out.detach(), xi.grad] + [p.grad.clone() for p in conv.parameters()]


def test_bdd_route_selection_and_fallback():
    G = _graph("edges")
    th.manual_seed(1)
    x, norm = th.randn(G.n, 32, device=DEV), th.rand(len(G.src), 1, device=DEV)
    shape = (G.R, 32, 16, 4)
    assert B.rgcn_bdd_route(G.g, x, shape, norm, G.t) is not None
    assert B.rgcn_bdd_route(G.g, x, shape, None, G.t) is not None
    g64 = dgl.DGLGraph(G.g._graph.asbits(64))
    ng = norm.clone().requires_grad_()
    wide = th.randn(G.n, 1024, device=DEV)
    assert B.rgcn_bdd_route(g64, x, shape, norm, G.t) is None
    assert B.rgcn_bdd_route(G.g, x, shape, ng, G.t) is None
    assert B.rgcn_bdd_route(G.g, wide, (G.R, 1024, 1024, 32), norm, G.t) is None   # in * s_o = 32768
    for g, xx, nn_, dims in ((g64, x, norm, (32, 16, 4)), (G.g, x, ng, (32, 16, 4)),
                             (G.g, wide, norm, (1024, 1024, 32))):
        conv = RelGraphConv(dims[0], dims[1], G.R, "bdd", dims[2], self_loop=True).to(DEV)
        a = _module_run(conv, g, xx, G.t, nn_, True)
        b = _module_run(conv, g, xx, G.t, nn_, False)
        assert all(th.equal(p, q) for p, q in zip(a, b))


def test_bdd_deterministic_on_the_hub():
    G = _graph("full")
    th.manual_seed(2)
    conv = RelGraphConv(20, 20, G.R, "bdd", 4, self_loop=True).to(DEV)
    x, norm = th.randn(G.n, 20, device=DEV), th.rand(len(G.src), 1, device=DEV)
    a = _module_run(conv, G.g, x, G.t, norm, True)
    b = _module_run(conv, G.g, x, G.t, norm, True)
    assert all(th.equal(p, q) for p, q in zip(a, b))


def test_bdd_module_matches_the_table_path():
    g, src, dst, et, n = typed_graph(seed=2)
    th.manual_seed(0)
    conv = RelGraphConv(32, 16, 4, "bdd", 4, self_loop=True).to(DEV)
    x, norm = th.randn(n, 32, device=DEV), th.rand(len(src), 1, device=DEV)
    etypes = th.from_numpy(et).to(DEV)
    assert B.rgcn_bdd_route(g, x, (4, 32, 16, 4), norm, etypes) is not None
    a = _module_run(conv, g, x, etypes, norm, True)
    b = _module_run(conv, g, x, etypes, norm, False)
    assert th.allclose(a[0], b[0], rtol=1e-4, atol=1e-3)
    for p, q in zip(a[1:], b[1:]):
        assert th.allclose(p, q, rtol=1e-3, atol=1e-2)


def test_bdd_builds_no_node_by_relation_table():
    n, R, f = 2000, 512, 64
    g, src, dst, et, n = typed_graph(n=n, m=20000, R=R, seed=3)
    th.manual_seed(0)
    conv = RelGraphConv(f, f, R, "bdd", 8).to(DEV)
    x, etypes = th.randn(n, f, device=DEV), th.from_numpy(et).to(DEV)
    assert B.rgcn_bdd_route(g, x, (R, f, f, 8), None, etypes) is not None
    th.cuda.synchronize()
    th.cuda.reset_peak_memory_stats()
    before = th.cuda.memory_allocated()
    _module_run(conv, g, x, etypes, None, True)
    th.cuda.synchronize()
    assert th.cuda.max_memory_allocated() - before < n * R * f * 4 / 4
