"""The fused GAT walks (csrc/kernels_gat.hip) at every lane configuration and at every chunk
length, against a dense fp64 restatement with derived bounds (needs an MI355X).  DESIGN.md
4.3-t has the derivations, the observed / bound ratios and the mutant table.

Lane configurations, by ``pick`` (restated here; if it changes, revisit SHAPES and
``_coverage``): a row of F = H D floats is F4 = F / 4 float4 slots, walked by a group of L
lanes with NV slots per lane -- (4,1) up to F4 = 4, (8,1), (16,1), (32,1), (64,1), (64,2) up
to F4 = 128 and (64,4) up to F4 = 256.  A head's D4 = D / 4 slots sit on adjacent lanes and
reduce by head_sum (two DPP rounds, then __shfl_xor from D4 = 8 on).

    A  every shape of SHAPES on test_fixup_segments_gpu.hub_edges (N = 512, K = 8 forward and
       backward: hub rows of 1, 1, 1, 2, 2, 3 and 33 fixup segments, rows that end on every
       position of a chunk), aligned / shifted / swapped; the forward with and without the
       slope aggregates, the three backward forms (DGLMI_GAT_SLOPES / DGLMI_GAT_EDGE_POS)
    B  one lane-filling shape per configuration at the smallest edge counts where a chunk of
       the forward and of the backward walk spans two or more full batches of B = max(L, 16)
       positions (LONG), and where the forward's chunk is exactly one batch (ONE_BATCH)
    C  column blocks (DGLMI_GAT_BLOCKS = 2, 3) on graph A with its destination rows spread over
       the id range (so that no block is empty), one shape per configuration
    D  bipartite blocks (700 -> 512 and 512 -> 700) passed straight to backend.fused_gat
    E  -inf / +inf / NaN logits in the forward on a small engineered graph

Chunk lengths by the rules at the time of writing (``fwd_chunk`` = gat_chunk_edges =
fast_chunk_edges(nnz, 64), ``bwd_chunk`` = gat_bwd_chunk_edges, restated below and asserted
per case).  If those rules change, revisit LONG, ONE_BATCH and the degree sets.

Reference: per-edge pre = el[u] + er[v] in fp64 from the fp32 inputs, s = leaky_relu(pre),
the row maximum (detached), exp, the attention scattered into a dense (N_dst, N_src, H)
tensor by index_add_ (parallel edges add), out = einsum(A, ft); gradients by autograd for a
CPU-drawn grad_out.  No (E, H, D) tensor is built.  The same dense tensors give the mass
A |ft|, the gradient majorants (sums of absolute values of every term), the degrees,
P = max |pre| and X = max |s - m| per row and head.

Bounds, u = 2^-24:

    out[v,h,:]   (6 deg_in(v) + 4 P + 2 X + 16 + extra) u mass      =: FF(v,h) u mass
    lf, ls       FF u (their own mass)
    g_ft[u]      u (sum_v A (FF(v) + 8) |go[v]|  +  2 deg_out(u) majorant)
    g_el[u]      u (sum_v W(v,u)  +  2 deg_out(u) majorant),   majorant = sum_v T(v,u)
    g_er[v]      u (sum_u W(v,u)  +  2 deg_in(v) majorant),    majorant = sum_u T(v,u)
    T = TG + TD,  TG = A lrelu' <|go|, |ft|>,  TD = A lrelu' <|go|, mass>,
    W = TG (FF(v) + D + 8) + TD (2 FF(v) + D + 8),  extra = 4 nb with nb column blocks

Every check requires finite values first (the direct calls start from NaN-filled buffers) and
counts anything not <= its bound as outside; rows without edges are exactly 0; every case run
twice is bit-equal; g_ft and g_el are bit-equal across the three backward forms.

DGLMI_GAT_SHAPES_DIGESTS=<file> writes a sha256 of every output of cases A-D (two library
builds compare bit for bit); ``pytest -s`` prints the observed / bound ratios.
"""
import contextlib
import hashlib
import json
import os
import zlib

import numpy as np
import pytest
import torch as th

import dgl
import dgl.backend as B
from dgl import kernel as K
from dgl.graph_index import device_block_gidx
from test_fixup_segments_gpu import HUB_DEGREES, hub_edges
from test_fixup_segments_gpu import N as NA
from test_fixup_segments_gpu import graph as hub_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
SLOPE = 0.2
VARIANTS = ("aligned", "shifted", "swapped")
CONFIGS = ((4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4))

SHAPES = {
    (4, 1): [(1, 4), (3, 4), (4, 4), (1, 16)],
    (8, 1): [(5, 4), (2, 16), (1, 32)],
    (16, 1): [(9, 4), (16, 4), (3, 16), (8, 8), (1, 64)],
    (32, 1): [(32, 4), (5, 16), (8, 16), (1, 128)],
    (64, 1): [(64, 4), (9, 16), (16, 16), (1, 256)],
    (64, 2): [(33, 8), (65, 4), (5, 64), (16, 32), (2, 256)],  # (65, 4): its D4 = 1 shape
    (64, 4): [(130, 4), (9, 64), (3, 256), (8, 128)],
}
# one lane-filling shape with H <= 8 per configuration (cases B, C, E)
FILL = {(4, 1): (4, 4), (8, 1): (2, 16), (16, 1): (8, 8), (32, 1): (8, 16), (64, 1): (4, 64),
        (64, 2): (8, 64), (64, 4): (8, 128)}
NB = 2048
# batch -> nnz: the smallest edge counts (+ 5: a partial last chunk, a masked last batch) where
# K forward = 4 B and K backward = 2 B, and where K forward = B
LONG = {16: (1 << 20) + 5, 32: (1 << 21) + 5, 64: (1 << 22) + 5}
ONE_BATCH = {16: (1 << 18) + 5, 32: (1 << 19) + 5, 64: (1 << 20) + 5}


def pick(F):
    """kernels_gat.hip pick(): (L, NV)."""
    for lim, cfg in zip((4, 8, 16, 32, 64, 128), CONFIGS):
        if F // 4 <= lim:
            return cfg
    return CONFIGS[-1]


def supported(H, D):
    """kernels_gat.hip gat_supported()."""
    d4 = D // 4
    return H >= 1 and D >= 4 and D % 4 == 0 and d4 & (d4 - 1) == 0 and H * D <= 1024 \
        and d4 <= pick(H * D)[0]


def fwd_chunk(nnz):
    """gat_chunk_edges = fast_chunk_edges(nnz, 64)."""
    k = 512
    while k > 8 and nnz // k < 256 * 64:
        k >>= 1
    return k


def bwd_chunk(nnz):
    """gat_bwd_chunk_edges: one more halving under 2 x 16 K groups."""
    k = fwd_chunk(nnz)
    return k >> 1 if k > 8 and nnz // k < 2 * 256 * 64 else k


def batch(cfg):
    return max(cfg[0], 16)


def _coverage():
    """What the module docstring promises, by pick's rule."""
    for cfg, shapes in SHAPES.items():
        L, NV = cfg
        assert all(supported(H, D) and pick(H * D) == cfg for H, D in shapes), cfg
        f4 = [H * D // 4 for H, D in shapes]
        d4 = [D // 4 for _, D in shapes]
        assert any(x == L * NV for x in f4), (cfg, "fills its lanes")
        assert any(x < L * NV for x in f4), (cfg, "idle slots")
        assert 1 in d4, (cfg, "D4 = 1")
        assert min(L, 64) in d4, (cfg, "D4 = L")
        assert supported(*FILL[cfg]) and pick(FILL[cfg][0] * FILL[cfg][1]) == cfg and FILL[cfg][0] <= 8
        assert FILL[cfg][0] * FILL[cfg][1] // 4 == L * NV
    assert 64 < 5 * 64 // 4 < 128 and (5, 64) in SHAPES[(64, 2)]      # a partly filled second slot
    assert 128 < 9 * 64 // 4 < 192 and (9, 64) in SHAPES[(64, 4)]     # partly filled third, idle fourth
    assert 3 * 256 // 4 == 192 and (3, 256) in SHAPES[(64, 4)]        # a wholly idle fourth slot
    na = len(hub_edges("aligned")[0])
    assert fwd_chunk(na) == 8 and bwd_chunk(na) == 8 and 31865 <= na < 40000
    for b in (16, 32, 64):
        assert fwd_chunk(LONG[b]) == 4 * b and bwd_chunk(LONG[b]) == 2 * b
        assert fwd_chunk(LONG[b] - 6) == 2 * b  # the smallest such count
        assert fwd_chunk(ONE_BATCH[b]) == b and fwd_chunk(ONE_BATCH[b] - 6) == b // 2


_coverage()

RATIOS = {}    # (config, output) -> max err / bound over every case
TIGHTER = {}   # output -> min over rows of in-degree <= 32 of (old band / bound)
DIGESTS = {}


def _seed(*key):
    return zlib.crc32(repr(key).encode()) % (2 ** 31)


def _rand(seed, *shape):
    """Fixed inputs drawn on the CPU (the same for every library build)."""
    x = np.random.RandomState(seed).uniform(-1.0, 1.0, shape).astype(np.float32)
    return th.from_numpy(x).to(DEV)


def _inputs(key, n_src, n_dst, H, D):
    s = _seed(key, H, D)
    return (_rand(s, n_src, H, D), _rand(s + 1, n_src, H, 1), _rand(s + 2, n_dst, H, 1),
            _rand(s + 3, n_dst, H, D))


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


def _within(cfg, name, got, exact, bound, tag):
    got = got.double().reshape(exact.shape)
    assert bool(th.isfinite(got).all()), "%s %s: %d of %d not finite (left unwritten?)" % (
        tag, name, int((~th.isfinite(got)).sum()), got.numel())
    err = (got - exact).abs()
    ratio = float((err / bound.clamp(min=1e-300)).max())
    RATIOS[(cfg, name)] = max(RATIOS.get((cfg, name), 0.0), ratio)
    bad = ~(err <= bound)  # a NaN anywhere counts as outside
    assert not bool(bad.any()), "%s %s: %d of %d outside, max err / bound %g (err %g)" % (
        tag, name, int(bad.sum()), bad.numel(), ratio, float(err.max()))


def _digest(tag, outs):
    if os.environ.get("DGLMI_GAT_SHAPES_DIGESTS"):
        for k, t in outs.items():
            DIGESTS["%s %s" % (tag, k)] = hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


# ---- the reference -------------------------------------------------------------------------
def reference(src, dst, n_src, n_dst, ft, el, er, go, extra=0):
    """src / dst: int64 device tensors.  Returns the exact values and the bounds of out, lf,
    ls, g_ft, g_el and g_er as a dict name -> (exact, bound), and the row degrees."""
    H, D = ft.shape[1], ft.shape[2]
    f, l, r = (t.double().requires_grad_() for t in (ft, el, er))
    pre = l[src, :, 0] + r[dst, :, 0]
    s = th.nn.functional.leaky_relu(pre, SLOPE)
    m = th.full((n_dst, H), -1e300, dtype=th.float64, device=DEV).index_reduce_(0, dst, s.detach(), "amax")
    ex = th.exp(s - m[dst])
    den = th.zeros(n_dst, H, dtype=th.float64, device=DEV).index_add_(0, dst, ex)
    a = ex / den[dst]
    A = th.zeros(n_dst * n_src, H, dtype=th.float64, device=DEV).index_add_(0, dst * n_src + src, a)
    A = A.view(n_dst, n_src, H)
    out = th.einsum("vuh,uhd->vhd", A, f)
    g_ft, g_el, g_er = th.autograd.grad(out, (f, l, r), go.double())
    with th.no_grad():
        zero = th.zeros(n_dst, H, dtype=th.float64, device=DEV)
        P = zero.clone().index_reduce_(0, dst, pre.abs(), "amax")
        X = zero.clone().index_reduce_(0, dst, (s - m[dst]).abs(), "amax")
        del pre, s, ex, a
        deg_in = th.bincount(dst, minlength=n_dst).double()
        deg_out = th.bincount(src, minlength=n_src).double()
        A = A.detach()
        af, ag, out = ft.double().abs(), go.double().abs(), out.detach()
        FF = 6 * deg_in[:, None] + 4 * P + 2 * X + 16 + extra              # (N_dst, H)
        mass = th.einsum("vuh,uhd->vhd", A, af)
        AS = A * ((l.detach()[None, :, :, 0] + r.detach()[:, None, :, 0] > 0).double() * (1 - SLOPE) + SLOPE)
        lf = th.einsum("vuh,uhd->vhd", AS, ft.double())
        lf_mass = th.einsum("vuh,uhd->vhd", AS, af)
        ls = AS.sum(1)
        # the terms of g_el / g_er: a lrelu' (<go, ft> - <go, out>), every product in magnitude
        # and weighted by what each part carries: the attention FF, its dot D + 8; the
        # <go, out> part the error of out as well, FF once more
        TG = AS * th.einsum("vhd,uhd->vuh", ag, af)
        TD = AS * (ag * mass).sum(-1)[:, None, :]
        del AS
        T = TG + TD
        W = TG * (FF + D + 8)[:, None, :] + TD * (2 * FF + D + 8)[:, None, :]
        del TG, TD
        maj_ft = th.einsum("vuh,vhd->uhd", A, ag)
        w_ft = th.einsum("vuh,vhd->uhd", A * (FF[:, None, :] + 8), ag)
        maj_el, w_el = T.sum(0), W.sum(0)
        maj_er, w_er = T.sum(1), W.sum(1)
        del T, W, A
        res = {
            "out": (out, FF[:, :, None] * U * mass),
            "lf": (lf, FF[:, :, None] * U * lf_mass),
            "ls": (ls, FF * U * ls),
            "g_ft": (g_ft, U * (w_ft + 2 * deg_out[:, None, None] * maj_ft)),
            "g_el": (g_el[:, :, 0], U * (w_el + 2 * deg_out[:, None] * maj_el)),
            "g_er": (g_er[:, :, 0], U * (w_er + 2 * deg_in[:, None] * maj_er)),
        }
    return res, deg_in, deg_out


# ---- the library ---------------------------------------------------------------------------
def _nan(*shape):
    return th.full(shape, float("nan"), device=DEV)


def forward(gidx, ft, el, er, slopes):
    n_dst, (H, D) = er.shape[0], ft.shape[1:]
    o = {"out": _nan(n_dst, H, D), "m": _nan(n_dst, H), "l": _nan(n_dst, H)}
    if slopes:
        o["lf"], o["ls"] = _nan(n_dst, H, D), _nan(n_dst, H)
    K.fused_gat_forward(gidx, ft, el, er, SLOPE, o["out"], o["m"], o["l"], o.get("lf"), o.get("ls"))
    return o


def backward(gidx, ft, el, er, fw, go, form):
    """form: "11" the slope aggregates' dense pass, "01" edge positions, "00" the destination walk."""
    g = {"g_ft": _nan(*ft.shape), "g_el": _nan(*el.shape), "g_er": _nan(*er.shape)}
    with _env(DGLMI_GAT_EDGE_POS=form[1]):
        K.fused_gat_backward(gidx, ft, el, er, SLOPE, fw["out"], fw["m"], fw["l"], go, g["g_ft"],
                             g["g_el"], g["g_er"], *((fw["lf"], fw["ls"]) if form == "11" else ()))
    return g


def run_all(gidx, ft, el, er, go, forms):
    """The forward with and without the slope aggregates and the backward forms."""
    with_ls = forward(gidx, ft, el, er, True)
    plain = forward(gidx, ft, el, er, False)
    res = {"out": with_ls["out"], "lf": with_ls["lf"], "ls": with_ls["ls"], "out_plain": plain["out"],
           "m": with_ls["m"], "l": with_ls["l"], "m_plain": plain["m"], "l_plain": plain["l"]}
    for form in forms:
        g = backward(gidx, ft, el, er, with_ls if form == "11" else plain, go, form)
        res.update({k + "_" + form: v for k, v in g.items()})
    th.cuda.synchronize()
    return res


def check_case(cfg, tag, gidx, src, dst, n_src, n_dst, H, D, forms, extra=0, autograd=True):
    assert pick(H * D) == cfg
    ft, el, er, go = _inputs(tag, n_src, n_dst, H, D)
    got = run_all(gidx, ft, el, er, go, forms)
    again = run_all(gidx, ft, el, er, go, forms)
    for k in got:
        assert th.equal(got[k], again[k]), "%s %s: two runs differ" % (tag, k)
    _digest("%s %dx%d" % (tag, H, D), got)
    # keeping the slope aggregates changes nothing else
    for k in ("out", "m", "l"):
        assert th.equal(got[k], got[k + "_plain"]), "%s %s: changed by keeping lf / ls" % (tag, k)
    ref, deg_in, deg_out = reference(src, dst, n_src, n_dst, ft, el, er, go, extra)
    for k in ("out", "lf", "ls"):
        _within(cfg, k, got[k], *ref[k], tag)
    for form in forms:
        for k in ("g_ft", "g_el", "g_er"):
            _within(cfg, k, got[k + "_" + form], *ref[k], "%s form %s" % (tag, form))
    for form in forms[1:]:
        for k in ("g_ft", "g_el"):
            assert th.equal(got[k + "_" + form], got[k + "_" + forms[0]]), \
                "%s %s: forms %s and %s differ" % (tag, k, form, forms[0])
    for k in ("out", "lf", "ls"):
        assert bool((got[k][deg_in == 0] == 0).all()), "%s %s: rows without in-edges" % (tag, k)
    for form in forms:
        assert bool((got["g_er_" + form][deg_in == 0] == 0).all()), tag
        assert bool((got["g_ft_" + form][deg_out == 0] == 0).all()), tag
        assert bool((got["g_el_" + form][deg_out == 0] == 0).all()), tag
    if autograd:
        # the autograd wrapper reaches the same entries: bit-equal to the direct calls
        with _env(DGLMI_GAT_SLOPES="1" if forms[0] == "11" else "0", DGLMI_GAT_EDGE_POS=forms[0][1]):
            leaves = [t.clone().requires_grad_() for t in (ft, el, er)]
            out = B.fused_gat(gidx, *leaves, SLOPE)
            gs = th.autograd.grad(out, leaves, go)
        assert th.equal(out.detach(), got["out"]), tag + ": backend.fused_gat out"
        for k, g in zip(("g_ft", "g_el", "g_er"), gs):
            assert th.equal(g, got[k + "_" + forms[0]]), "%s: backend.fused_gat %s" % (tag, k)
    return ref, deg_in, deg_out


def _tighter(ref, deg_in, deg_out, D):
    """How much tighter than the earlier bands (rtol = atol = 1e-4 for out, 1e-3 for the
    gradients) the bounds are on rows of degree <= 32 of the walk that owns them (in-degree for
    out and g_er, out-degree for g_ft and g_el): the least (band + band |ref|) / bound over
    their elements, recorded per D.  out's mass is a weighted mean of |ft| whatever D is: at
    least 10 x, asserted, as is g_ft's (a weighted sum of |go| rows).  The logit gradients'
    bounds do not reach 10 x beyond D = 4: their majorant is a sum of D-term
    dots and grows with D while the earlier band was absolute, and a low-degree source carries
    the forward factor of the hub rows it points at; g_el and g_er are asserted at D = 4, the
    rest is recorded."""
    for names, deg, band in ((("out",), deg_in, 1e-4), (("g_er",), deg_in, 1e-3),
                             (("g_ft", "g_el"), deg_out, 1e-3)):
        rows = (deg > 0) & (deg <= 32)
        if not bool(rows.any()):
            continue
        for k in names:
            exact, bound = ref[k]
            t = float(((band + band * exact[rows].abs()) / bound[rows].clamp(min=1e-300)).min())
            TIGHTER[(k, D)] = min(TIGHTER.get((k, D), float("inf")), t)
            if k in ("out", "g_ft") or D == 4:
                assert t >= 10.0, "%s: only %.1f x tighter than the %g band on rows of degree <= 32" % (k, t, band)


def _ends(variant):
    _, s, d = hub_graph(variant)
    return s.long(), d.long()


def _gidx(variant):
    return hub_graph(variant)[0]._graph.get_immutable_gidx(DEV)


# ---- A: every configuration on the segment-boundary graph ----------------------------------
A_CASES = [(cfg, H, D, v) for cfg in CONFIGS for (H, D) in SHAPES[cfg] for v in VARIANTS]


@pytest.mark.parametrize("cfg,H,D,variant", A_CASES,
                         ids=["L%dx%d-%dx%d-%s" % (c + (h, d, v)) for c, h, d, v in A_CASES])
def test_every_shape_on_segment_boundaries(cfg, H, D, variant):
    src, dst = _ends(variant)
    assert HUB_DEGREES[-1] == 8 * 1025 + 1  # 33 fixup segments at K = 8
    gidx = _gidx(variant)
    ref, deg_in, deg_out = check_case(cfg, "A %s" % variant, gidx, src, dst, NA, NA, H, D, ("11", "01", "00"))
    assert getattr(gidx, "_gat_pos", None) is not None  # the edge-position path ran
    _tighter(ref, deg_in, deg_out, D)


# ---- B: long chunks -------------------------------------------------------------------------
_GRAPHS = {}


def long_graph(nnz, b, swapped):
    """Destination degrees: 0 1 2 3, B - 1 B B + 1, K - 1 K K + 1 for both chunk lengths,
    2 K + 1 and 33 K + 1 (two fixup segments at the forward's K), each once on a chunk boundary
    and once one position after it; fillers to the count; uniform sources; shuffled edge ids."""
    key = (nnz, swapped)
    if key not in _GRAPHS:
        kf, kb = fwd_chunk(nnz), bwd_chunk(nnz)
        special = [0, 1, 2, 3, b - 1, b, b + 1, kb - 1, kb, kb + 1, kf - 1, kf, kf + 1,
                   2 * kb + 1, 2 * kf + 1, 33 * kf + 1]
        rs = np.random.RandomState(nnz % 65521)
        deg, pos = [], 0
        for off in (0, 1):
            for d in special:
                pad = (off - pos) % kf
                deg += [pad, d]
                pos += pad + d
                assert (pos - d) % kf == off
        rest = NB - len(deg)
        assert rest > 0 and nnz - pos > rest
        deg = np.array(deg + list(rs.multinomial(nnz - pos, np.full(rest, 1.0 / rest))))
        dst = np.repeat(np.arange(NB), deg)
        src = rs.randint(0, NB, nnz)
        perm = rs.permutation(nnz)
        src, dst = src[perm], dst[perm]
        if swapped:
            src, dst = dst, src
        s, d = th.from_numpy(src).to(DEV), th.from_numpy(dst).to(DEV)
        g = dgl.DGLGraph.from_device_coo(s.int(), d.int(), NB)
        _GRAPHS[key] = (g._graph.get_immutable_gidx(DEV), s, d)
    return _GRAPHS[key]


B_CASES = [(cfg, table, sw) for table in ("long", "one_batch") for cfg in CONFIGS for sw in (False, True)
           if table == "long" or not sw]


@pytest.mark.parametrize("cfg,table,swapped", B_CASES,
                         ids=["L%dx%d-%s-%s" % (c + (t, "swapped" if s else "in")) for c, t, s in B_CASES])
def test_long_chunks(cfg, table, swapped):
    b = batch(cfg)
    nnz = (LONG if table == "long" else ONE_BATCH)[b]
    if table == "long":
        assert fwd_chunk(nnz) >= 2 * b and bwd_chunk(nnz) >= 2 * b
    else:
        assert fwd_chunk(nnz) == b
    gidx, src, dst = long_graph(nnz, b, swapped)
    assert gidx.in_csr.nnz == nnz
    H, D = FILL[cfg]
    check_case(cfg, "B %s %s" % (table, "swapped" if swapped else "in"), gidx, src, dst, NB, NB, H, D,
               ("11", "00"), autograd=table == "long")


# ---- C: column blocks -----------------------------------------------------------------------
@pytest.mark.parametrize("slopes", ["1", "0"])
@pytest.mark.parametrize("nb", [2, 3])
@pytest.mark.parametrize("cfg", CONFIGS, ids=["L%dx%d" % c for c in CONFIGS])
def test_column_blocks(cfg, nb, slopes):
    """Graph A (aligned) with destination row i renamed 10 i: the rows keep their order, degrees
    and starts, and the out-CSR's blocks (by destination range) all hold edges -- the library
    walks unblocked when a block on either side is empty, and A's destinations are rows 0..49."""
    if "C" not in _GRAPHS:
        src, dst = hub_edges("aligned")
        assert dst.max() < 2 * len(HUB_DEGREES) <= NA // 10
        s, d = th.from_numpy(src).to(DEV), th.from_numpy(10 * dst).to(DEV)
        _GRAPHS["C"] = (device_block_gidx(NA, NA, s.int(), d.int()), s, d)
    gidx, src, dst = _GRAPHS["C"]
    ptr = gidx.in_csr.indptr[10 * (2 * th.arange(len(HUB_DEGREES), device=DEV) + 1)]
    assert bool((ptr % 64 == 0).all())  # the hub rows still start on multiples of 64
    ib, ob = gidx.col_blocks(nb)
    assert len(ib) == nb and all(c.nnz > 0 for c in ib + ob) and sum(c.nnz for c in ib) == len(src)
    H, D = FILL[cfg]
    with _env(DGLMI_GAT_BLOCKS=str(nb)):
        assert K.gat_col_blocks(gidx, th.empty(NA, H, D)) == nb
        check_case(cfg, "C nb%d" % nb, gidx, src, dst, NA, NA, H, D, ("11",) if slopes == "1" else ("00",),
                   extra=4 * nb)


# ---- D: bipartite ---------------------------------------------------------------------------
@pytest.mark.parametrize("H,D", [(8, 8), (5, 16), (9, 64)])
@pytest.mark.parametrize("n_src,n_dst", [(700, 512), (512, 700)])
def test_bipartite(n_src, n_dst, H, D):
    """A's degree structure on the smaller side (hubs as destinations for 700 -> 512, as
    sources for 512 -> 700), the other ends uniform over the larger side."""
    u, v = hub_edges("shifted")
    rs = np.random.RandomState(11)
    if n_dst == 512:
        src, dst = rs.randint(0, n_src, len(v)), v
    else:
        src, dst = v, rs.randint(0, n_dst, len(v))
    s, d = th.from_numpy(src).to(DEV), th.from_numpy(dst).to(DEV)
    gidx = device_block_gidx(n_src, n_dst, s.int(), d.int())
    ref, _, _ = check_case(pick(H * D), "D %d->%d" % (n_src, n_dst), gidx, s, d, n_src, n_dst, H, D,
                        ("11", "01", "00"))
    assert ref["g_ft"][0].shape[0] == n_src and ref["g_er"][0].shape[0] == n_dst


# ---- E: special logits, forward -------------------------------------------------------------
NE = 512
INF = float("inf")
HUB_E = 8 * 40 + 3  # 40 continuation chunks at K = 8: two fixup segments
SPREAD = 34


def special_graph():
    """Rows (their sources ascending, which is the in-CSR's order within a row):
    0-2 short rows with a -inf source first / last / in the middle, 3 fed by -inf sources only,
    4 cut by chunks (a -inf source first in a continuation chunk, one mid-chunk, one last),
    5 a hub of two fixup segments (first, last and one whole chunk piece -inf), 6 a +inf source,
    7 a NaN source, 8 a NaN destination, 9-12 clean rows (short, cut, empty, cut), 13 three -inf
    sources below 256 and two finite ones above, 14 two -inf sources on either side of 256 (with
    two column blocks: a block that sees only masked edges of a row whose other block is finite
    / masked too).  Row i has the id SPREAD i: the rows keep their order and positions, and
    both halves of the destination range hold edges (the library walks unblocked otherwise)."""
    rows = {0: range(10, 13), 1: range(13, 16), 2: range(16, 21), 3: range(21, 26), 4: range(30, 51),
            5: range(60, 60 + HUB_E), 6: range(400, 403), 7: range(403, 406), 8: range(406, 408),
            9: range(420, 424), 10: range(424, 441), 12: range(441, 450),
            13: [52, 53, 54, 390, 391], 14: [55, 56, 392, 393]}
    src = np.concatenate([np.array(list(v)) for v in rows.values()])
    dst = np.concatenate([np.full(len(v), SPREAD * k) for k, v in rows.items()])
    perm = np.random.RandomState(3).permutation(len(src))
    return src[perm], dst[perm]


def _special_reference(src, dst, ft, el, er, extra=0):
    """Dense fp64, -inf / +inf / NaN carried as IEEE does: returns out, the bound of its finite
    elements, and the in-degrees."""
    H = ft.shape[1]
    cnt = th.zeros(NE * NE, dtype=th.float64, device=DEV).index_add_(
        0, dst * NE + src, th.ones(len(src), dtype=th.float64, device=DEV)).view(NE, NE, 1)
    pre = el.double()[None, :, :, 0] + er.double()[:, None, :, 0]          # (v, u, h)
    s = th.where(pre > 0, pre, SLOPE * pre)
    edge = (cnt > 0).expand(NE, NE, H)
    m = th.where(edge, s, th.full_like(s, -INF)).amax(1, keepdim=True)      # NaN propagates
    w = th.where(edge, cnt * th.exp(s - m), th.zeros_like(s))
    A = th.where(edge, w / w.sum(1, keepdim=True), th.zeros_like(s))  # a row without edges: 0
    out = th.einsum("vuh,uhd->vhd", A, ft.double())
    deg = cnt.sum((1, 2))
    fin = th.isfinite(pre) & edge
    P = th.where(fin, pre.abs(), th.zeros_like(s)).amax(1)
    X = th.where(fin, (s - m).abs(), th.zeros_like(s)).amax(1)
    X = th.where(th.isfinite(X), X, th.zeros_like(X))
    mass = th.einsum("vuh,uhd->vhd", th.where(th.isfinite(A), A, th.zeros_like(A)), ft.double().abs())
    return out, (6 * deg[:, None] + 4 * P + 2 * X + 16 + extra)[:, :, None] * U * mass, deg


def _special_inputs(gidx, H, D):
    """(ft, el, er) with the special values on every other head, the same with 0.25 in their
    place, and the (row, head) pairs a special value reaches."""
    ft, el, er, _ = _inputs("E", NE, NE, H, D)
    full = gidx.in_csr.indptr.cpu().numpy().astype(np.int64)
    idx = gidx.in_csr.indices.cpu().numpy().astype(np.int64)
    assert fwd_chunk(len(idx)) == 8
    ptr = full[SPREAD * np.arange(16)]  # ptr[i]: where row i (id SPREAD i) starts
    assert (np.diff(ptr) == [3, 3, 5, 5, 21, HUB_E, 3, 3, 2, 4, 17, 0, 9, 5, 4]).all() and ptr[15] == len(idx)
    for r in range(15):
        assert (np.diff(idx[ptr[r]:ptr[r + 1]]) > 0).all()  # sources ascending: positions are known
    assert ptr[4] % 8 == 0
    first_cont = ptr[4] + 8                       # row 4: the first position of its second chunk
    piece = (ptr[5] // 8 + 6) * 8                 # row 5: one whole chunk piece past the head's
    assert ptr[5] % 8 != 0 and ptr[5] < piece and piece + 8 < ptr[6]
    minus = [idx[ptr[0]], idx[ptr[1 + 1] - 1], idx[ptr[2] + 2]] + list(idx[ptr[3]:ptr[4]]) + \
        [idx[first_cont], idx[first_cont + 3], idx[ptr[5] - 1]] + \
        [idx[ptr[5]], idx[ptr[6] - 1]] + list(idx[piece:piece + 8]) + [52, 53, 54, 55, 56, 392, 393]
    heads = list(range(0, H, 2))
    minus = th.tensor([int(x) for x in minus], device=DEV)
    el2, er2 = el.clone(), er.clone()
    for h in heads:
        el2[minus, h] = -INF
        el2[401, h] = INF
        el2[404, h] = float("nan")
        er2[SPREAD * 8, h] = float("nan")
    plain_el = th.where(th.isfinite(el2), el2, th.full_like(el2, 0.25))
    plain_er = th.where(th.isfinite(er2), er2, th.full_like(er2, 0.25))
    touched = th.zeros(NE, H, dtype=th.bool, device=DEV)
    for r in list(range(9)) + [13, 14]:
        touched[SPREAD * r, heads] = True
    return ft, el2, er2, plain_el, plain_er, touched


E_CASES = [(cfg, 1) for cfg in CONFIGS] + [((16, 1), 2)]  # column blocks (k_gat_merge) at one shape


@pytest.mark.parametrize("cfg,nb", E_CASES, ids=["L%dx%d-nb%d" % (c + (n,)) for c, n in E_CASES])
def test_special_logits_forward(cfg, nb):
    """A -inf logit has weight 0 wherever it sits (first in a row, first in a continuation
    chunk, a whole chunk piece of a hub); a row with edges that is masked everywhere, and a row
    that meets +inf or NaN, is NaN as in the fp64 restatement and the edge-softmax entries; a row
    without edges is exactly 0; rows and heads no special value reaches do not change a bit."""
    H, D = FILL[cfg]
    src, dst = special_graph()
    s, d = th.from_numpy(src).to(DEV), th.from_numpy(dst).to(DEV)
    gidx = device_block_gidx(NE, NE, s.int(), d.int())
    ft, el, er, pel, per, touched = _special_inputs(gidx, H, D)
    ref, bound, deg = _special_reference(s, d, ft, el, er, extra=4 * nb if nb > 1 else 0)
    nan_rows = th.isnan(ref).any(-1)
    expect = th.zeros(NE, H, dtype=th.bool, device=DEV)
    for r in (3, 6, 7, 8, 14):
        expect[SPREAD * r, 0::2] = True
    assert th.equal(nan_rows, expect)  # the reference: masked everywhere, +inf, NaN, NaN, masked
    if nb > 1:  # the blocks are in use, and they cut rows 5, 13 and 14
        ib, ob = gidx.col_blocks(nb)
        assert len(ib) == nb and all(c.nnz > 0 for c in ib + ob) and sum(c.nnz for c in ib) == len(src)
        per_block = [[int(c.indptr[SPREAD * r + 1] - c.indptr[SPREAD * r]) for c in ib] for r in (3, 5, 13, 14)]
        assert per_block == [[5, 0], [256 - 60, 60 + HUB_E - 256], [3, 2], [2, 2]], per_block
    with _env(DGLMI_GAT_BLOCKS=str(nb)):
        assert K.gat_col_blocks(gidx, ft) == nb
        for slopes in (False, True):
            got = forward(gidx, ft, el, er, slopes)
            base = forward(gidx, ft, pel, per, slopes)
            th.cuda.synchronize()
            tag = "E %s slopes %d" % (cfg, slopes)
            out = got["out"].double()
            pattern = th.isnan(out)
            assert th.equal(pattern, th.isnan(ref)), "%s: NaN at %s, expected at %s" % (
                tag, sorted({r // SPREAD for r in pattern.any(-1).nonzero()[:, 0].tolist()}),
                sorted({r // SPREAD for r in nan_rows.nonzero()[:, 0].tolist()}))
            ok = ~th.isnan(ref)
            assert bool(th.isfinite(out[ok]).all()), tag
            err = (out[ok] - ref[ok]).abs()
            lim = bound[ok]
            assert bool((err <= lim).all()), "%s: max err / bound %g" % (tag, float((err / lim.clamp(min=1e-300)).max()))
            assert bool((got["out"][deg == 0] == 0).all()), tag + ": rows without edges"
            for k in got:
                assert th.equal(got[k][~touched], base[k][~touched]), "%s %s: untouched rows / heads changed" % (tag, k)


def test_zz_report():
    """Prints what DESIGN.md 4.3-t tabulates (pytest -s); writes the digests when asked."""
    for cfg in CONFIGS:
        row = ["%s %.3f" % (k, RATIOS[(cfg, k)]) for k in ("out", "lf", "ls", "g_ft", "g_el", "g_er")
               if (cfg, k) in RATIOS]
        print("max err / bound, (L, NV) = %s: %s" % (cfg, "  ".join(row)))
    print("earlier band / bound on rows of degree <= 32, least:",
          "  ".join("%s D=%d %.1f" % (k + (v,)) for k, v in sorted(TIGHTER.items())))
    path = os.environ.get("DGLMI_GAT_SHAPES_DIGESTS")
    if path:
        with open(path, "w") as f:
            json.dump(DIGESTS, f, indent=0, sort_keys=True)
