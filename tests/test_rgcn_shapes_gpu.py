"""The R-GCN layer kernels of csrc/hack_kernels.hip -- k_gemm, k_gemm_rows<8,64 / 4,128 /
2,256>, k_gemm_tn<2,8 / 2,10 / 4,4 / 8,2>, k_rgcn_fused<BWD, 1 / 2 / 4> and
k_rgcn_fused16<BWD, 2 / 4 / 8> -- through the C entries, at every instance and at the
row counts, widths and edge layouts where they can go wrong.  EXACT, not close.

Method.  Every input is integer-valued: hidden in [-2, 2], relation and self-loop weights
in {-1, 0, 1}, norm in {1, 2}, grad_out / bias / addend in [-4, 4].  The fp32 MFMA
instructions are fused-multiply-add chains and the reduce kernels only add, so while the
absolute mass of a sum (the same sum over absolute values) stays below 2^24 every partial
sum is an integer fp32 holds exactly, in any order: each result must EQUAL (th.equal) the
float64 reference cast to fp32, on every route, and the fused and unfused results of one
call must equal each other.  Every test asserts max mass < 2^24 before it compares: a
condition on its inputs, not a tolerance.

Guard rows.  hidden and grad_out are the first n rows of buffers with 16 NaN tail rows;
every output is the head of a buffer pre-filled with a sentinel no integer equals.  After
the call the tail is still the sentinel bit for bit and no output element is.

Routes.  The unfused entries (capi.cpp rgcn_layer1_impl / rgcn_layer1_backward_impl) issue,
for N nodes and weights (R, F_in, F_out):
  forward          (N x F_in) . (F_in x R F_out)
  grad_hidden      (N x R F_out) . W_cat^T, B strides (1, R F_out)
  weight gradient  hidden^T . gy, A strides (1, F_in), DGLMIRgcnGemmSplits(F_in, R F_out, N)
  self-loop        hidden . loop, grad_out . loop^T, hidden^T . grad_out
Each case asserts through DGLMIRgcnGemmInstance / DGLMIRgcnFusedInstance that the kernel
it names is the one selected.  What ran where, N >= 4096 (below it every product is
k_gemm: rows needs M >= 4096, tn needs K >= 4096):

  (F_in, R, F_out)  forward     grad_hidden  weight grad  loop fwd    loop gh     loop gw
  (64, 4, 64)       rows<8,64>  rows<2,256>  tn<2,8>      rows<8,64>  rows<8,64>  tn<2,8>
  (4, 1, 1)         rows<8,64>  k_gemm       k_gemm       rows<8,64>  k_gemm      k_gemm
  (60, 5, 50)       rows<8,64>  k_gemm       k_gemm       rows<8,64>  k_gemm      k_gemm
  (128, 2, 64)      rows<4,128> rows<4,128>  tn<4,4>      rows<4,128> rows<8,64>  tn<4,4>
  (68, 3, 11)       rows<4,128> k_gemm       k_gemm       rows<4,128> k_gemm      k_gemm
  (256, 2, 32)      rows<2,256> rows<8,64>   tn<8,2>      rows<2,256> rows<8,64>  tn<8,2>
  (132, 1, 33)      rows<2,256> k_gemm       k_gemm       rows<2,256> k_gemm      k_gemm
  (64, 5, 64)       k_gemm      k_gemm       tn<2,10>     rows<8,64>  rows<8,64>  tn<2,8>
  (128, 4, 64)      k_gemm      k_gemm       k_gemm x8    rows<4,128> rows<8,64>  tn<4,4>
  (30, 2, 7)        k_gemm      k_gemm       k_gemm       k_gemm      k_gemm      k_gemm
  (260, 1, 16)      k_gemm      k_gemm       k_gemm       k_gemm      k_gemm      k_gemm

("k_gemm x8": split-K over 8 ranges with a column-major A.)  k_gemm_rows cannot take the
weight gradient (A is column-major there) and k_gemm_tn cannot take the other two (A is
row-major), so those are all the roles.  The fused walks run forward (F_in = 64, widths
F_out) and backward (F_out = 64, widths F_in) at widths 1, 31, 32 (one 32-column block),
33, 64 (two), 65, 127, 128 (four), on 16- and 32-row tiles: all twelve instances.  Behind
the fused backward one product hidden^T . gy (F_in x 64 (R + self-loop) over N) gives every
weight gradient; each fused case names its kernel too (tn<2,8>, tn<2,10>, tn<4,4> or
k_gemm).  DGLMIRgcnFusedInstance answers for the shape only: that the entry took the fused
walk rests on the state's matches() and the alignment assertions here, and since fused and
unfused results are both exact, a silent fall-back to the unfused path would pass.

k_gemm_tn tails.  launch_tn cuts the N node rows into blocks of rpb = ceil(N / s) rounded
up to 32, s = the split count, and runs ceil(N / rpb) of them.  gemm_splits keeps
512 <= N / s < 1024, so s rpb - N < 32 s: while 32 s < rpb all s blocks run and the last
holds more than rpb - 32 s rows.  At s = 8 (4096 <= N < 8192) that is more than 256 rows;
at s = 16 (N >= 8192) the smallest last block is 33 rows, at N = 8193 (rpb = 544): one
full 32-row slice and a one-row slice.  So no last block of a single row or a single
slice exists at s = 8 or 16.  From s = 32 (N >= 16384) on, 32 s exceeds rpb and any
remainder occurs: N = 16865 (rpb = 544, 31 * 544 = 16864) leaves a last block of exactly
one row, N = 16896 one of exactly 32 rows -- the kernel's nsl == 1 path (no second load,
the two-step loop not entered, only the tail step), with a partial and a full slice.  The
file runs N = 16865 and 16896, N = 8193 (a two-slice last block ending in a single row),
N = 4129 (s = 8, rpb = 544, 17 slices per block -- an odd count -- and a last block of 321
rows: 11 slices, the last of one row) and N = 4096 (rpb = 512: an even count, every slice
full), each on all four instances.

The norm "gathered by edge id" is reached with a state prepared without a norm: the
Python wrapper re-gathers the cached copies for any other norm tensor
(RgcnState.sync_norm), so a state built from another tensor would stream again.
"""
import functools

import numpy as np
import pytest
import torch as th

from dgl import _ffi
from dgl import kernel as K
from dgl.graph_index import device_block_gidx
from graphs import powerlaw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 16          # guard rows behind hidden / grad_out (NaN) and every output (sentinel)
SENT = -12345.5   # every exact result is an integer
LIMIT = float(2 ** 24)

K_GEMM, ROWS_8_64, ROWS_4_128, ROWS_2_256, TN_2_8, TN_2_10, TN_4_4, TN_8_2 = range(8)


# --------------------------------------------------------------------------- #
# graphs from a degree table
# --------------------------------------------------------------------------- #
def _row(pos, deg, base=0):
    t = [base] * 16
    t[pos] = deg
    return t


# edges per row of one 16-row tile and one relation
PATTERNS = [
    ("none", [0] * 16),                               # the relation absent from the tile
    ("one-last", _row(15, 1)),                        # one edge, in the tile's last row
    ("two-one-row", _row(6, 2)),                      # shares of one edge, two empty
    ("three-rows", [1, 0, 0, 0, 0, 1, 0, 0, 0, 1] + [0] * 6),  # an empty fourth share
    ("four-one-row", _row(3, 4)),                     # three carries into one row
    ("lone-64", _row(7, 64)),                         # shares of exactly 16
    ("lone-65", _row(8, 65)),                         # shares of 17: a second batch of one
    ("hub-200", _row(5, 200, base=1)),                # groups whose whole share is in the row
    ("spans-three", [0] * 4 + [3, 30, 3] + [0] * 9),  # a row over all four shares, rows around
    ("ones", [1] * 16),
    ("fives", [5] * 16),
    ("zero-seven", [0, 7] * 8),
    ("eights", [8] * 16),                             # share boundaries on row boundaries
]
# the patterns back to back (pairs share a 32-row tile), then each followed by an empty
# tile (alone in its 32-row tile)
LAYOUT = [p for _, p in PATTERNS] + [t for _, p in PATTERNS for t in (p, [0] * 16)]
SPAN = 16 * len(LAYOUT)
DST0, SRC0 = 64, 1024   # first designed destination row / source row (32-row aligned)
assert DST0 + SPAN <= SRC0 and DST0 % 32 == 0 and SRC0 % 32 == 0


def _designed(start, R):
    """(rows, relations) of the laid-out tables: tile i at rows start + 16 i, relation
    i % R."""
    rows, rels = [], []
    for i, table in enumerate(LAYOUT):
        for r, deg in enumerate(table):
            rows += [start + 16 * i + r] * deg
            rels += [i % R] * deg
    return np.asarray(rows, np.int64), np.asarray(rels, np.int64)


class _Graph:
    pass


@functools.lru_cache(maxsize=None)
def _graph(n_src, n_dst, R, m, seed):
    """A typed multigraph: the degree tables laid out on the destination side at rows
    DST0.. (the forward's relation-major in-CSR walk) and on the source side at rows
    SRC0.. (the backward's relation-major out-CSR walk), with random other endpoints that
    repeat (source, destination, relation) triples; the rest a power-law graph with a hub
    source, kept off the designed rows.  Graphs too small for the tables are random.
    Edge ids are shuffled."""
    rng = np.random.default_rng(seed)
    designed = n_dst >= DST0 + SPAN and n_src >= SRC0 + SPAN
    if designed:
        free_dst = np.setdiff1d(np.arange(n_dst), np.arange(DST0, DST0 + SPAN))
        free_src = np.setdiff1d(np.arange(n_src), np.arange(SRC0, SRC0 + SPAN))
        d1, t1 = _designed(DST0, R)
        pool = rng.choice(free_src, 24)  # few sources: repeated triples
        s1 = np.where(rng.random(len(d1)) < 0.5, rng.choice(pool, len(d1)), rng.choice(free_src, len(d1)))
        s2, t2 = _designed(SRC0, R)
        pool = rng.choice(free_dst, 24)
        d2 = np.where(rng.random(len(s2)) < 0.5, rng.choice(pool, len(s2)), rng.choice(free_dst, len(s2)))
        _, pd, _ = powerlaw(len(free_dst), m, seed=seed)
        d3 = free_dst[pd]
        s3 = free_src[rng.integers(0, len(free_src), m)]
        s3[: m // 10] = s3[0]   # a hub source: thousands of out-edges
        t3 = rng.integers(0, R, m)
        src, dst, et = (np.concatenate(x) for x in ((s1, s2, s3), (d1, d2, d3), (t1, t2, t3)))
    else:
        src, dst, et = rng.integers(0, n_src, m), rng.integers(0, n_dst, m), rng.integers(0, R, m)
        src[: m // 10] = src[0]
    perm = rng.permutation(len(src))
    src, dst, et = src[perm], dst[perm], et[perm]
    if designed:
        # the tables are what the relation-major walks will see
        for ids, start, n in ((dst, DST0, n_dst), (src, SRC0, n_src)):
            deg = np.bincount(et * n + ids, minlength=R * n).reshape(R, n)[:, start:start + SPAN]
            for i, table in enumerate(LAYOUT):
                for t in range(R):
                    want = table if t == i % R else [0] * 16
                    assert deg[t, 16 * i:16 * i + 16].tolist() == want, (i, t)
        assert len(set(zip(src.tolist(), dst.tolist(), et.tolist()))) < len(src)
    g = _Graph()
    g.n_src, g.n_dst, g.R, g.m = n_src, n_dst, R, len(src)
    g.s, g.d, g.et = (th.from_numpy(a).to(DEV) for a in (src, dst, et))
    g.et32 = g.et.int()
    g.norm = th.from_numpy(rng.integers(1, 3, (len(src), 1))).float().to(DEV)
    g.gidx = device_block_gidx(n_src, n_dst, g.s.int(), g.d.int())
    return g


def _square(n, R, m=30000, seed=7):
    return _graph(n, n, R, m, seed)


def _state(G, layers, cached=True):
    """Drop the graph's prepared state; build one for `layers` (0: none), with the norm
    cached (streamed in position order) or not (gathered by edge id)."""
    G.gidx.__dict__.pop("_rgcn_state", None)
    if layers:
        K.rgcn_prepare(G.gidx, G.norm if cached else None, G.R, layers=layers, etypes=G.et32)
        assert G.gidx._rgcn_state.matches(G.et32, G.R, 1 if layers & 6 else 0)


# --------------------------------------------------------------------------- #
# inputs, guards, references
# --------------------------------------------------------------------------- #
def _ints(gen, shape, lo, hi):
    return th.randint(lo, hi + 1, shape, device=DEV, generator=gen).float()


def _guarded(gen, n, f, lo, hi, offset=0):
    """The first n rows of an (n + PAD, f) integer buffer whose tail rows are NaN;
    offset = 1: a contiguous view 4 bytes into a NaN-filled buffer."""
    flat = th.full((offset + (n + PAD) * f + 3,), float("nan"), device=DEV)
    x = flat[offset:offset + n * f].view(n, f)
    x.copy_(_ints(gen, (n, f), lo, hi))
    assert x.is_contiguous() and x.data_ptr() % 16 == 4 * offset
    return x


def _out(*shape):
    """(buffer, view): the view is the head of a sentinel-filled buffer with PAD more rows."""
    numel = int(np.prod(shape))
    buf = th.full((numel + PAD * shape[-1],), SENT, device=DEV)
    return buf, buf[:numel].view(*shape)


def _guards_ok(*pairs):
    for buf, view in pairs:
        tail = buf[view.numel():]
        assert th.equal(tail.view(th.int32), th.full_like(tail, SENT).view(th.int32))
        assert bool((view != SENT).all())


def _inputs(G, fi, fo, seed, loop=False, offset=0):
    gen = th.Generator(device=DEV).manual_seed(seed)
    x = _Graph()
    x.fi, x.fo = fi, fo
    x.h = _guarded(gen, G.n_src, fi, -2, 2, offset)
    x.go = _guarded(gen, G.n_dst, fo, -4, 4)
    x.w = _ints(gen, (G.R, fi, fo), -1, 1)
    x.lw = _ints(gen, (fi, fo), -1, 1) if loop else None
    x.bias = _ints(gen, (fo,), -4, 4) if loop else None
    x.add = _ints(gen, (G.n_dst, fo), -4, 4) if loop else None
    return x


def _reference(G, x):
    """fp64 index_add_ / einsum on the device, with the absolute mass of every sum
    asserted below 2^24; returns (ret, grad_hidden, grad_weight, grad_loop) as fp32."""
    nrm = G.norm.double()

    def fwd(h, w, lw, bias, add):
        y = th.einsum("nk,rkx->rnx", h, w)
        out = th.zeros(G.n_dst, x.fo, dtype=th.float64, device=DEV).index_add_(
            0, G.d, y[G.et, G.s] * nrm)
        if lw is not None:
            out = out + h @ lw + bias + add
        return out

    def bwd(h, w, go, lw):
        gt = th.zeros(G.R * G.n_src, x.fo, dtype=th.float64, device=DEV).index_add_(
            0, G.et * G.n_src + G.s, go[G.d] * nrm).view(G.R, G.n_src, x.fo)
        gh = th.einsum("rnx,rkx->nk", gt, w)
        gw = th.einsum("nk,rnx->rkx", h, gt)
        if lw is None:
            return gh, gw, None
        return gh + go @ lw.t(), gw, h.t() @ go

    args = [t if t is None else t.double() for t in (x.h, x.w, x.lw, x.bias, x.add, x.go)]
    h, w, lw, bias, add, go = args
    ab = [t if t is None else t.abs() for t in args]
    ref = (fwd(h, w, lw, bias, add),) + bwd(h, w, go, lw)
    mass = (fwd(*ab[:5]),) + bwd(ab[0], ab[1], ab[5], ab[2])
    worst = max(float(t.max()) for t in mass if t is not None)
    print("max absolute mass %.4g (limit 2^24 = %.4g)" % (worst, LIMIT))
    assert worst < LIMIT
    return tuple(t if t is None else t.float() for t in ref)


def _forward(G, x):
    rb, ret = _out(G.n_dst, x.fo)
    if x.lw is None:
        K.rgcn_layer1(G.gidx, x.h, x.w, G.norm, ret, etypes=G.et32)
    else:
        K.rgcn_layer1_ex(G.gidx, x.h, x.w, G.norm, ret, loop_weight=x.lw, bias=x.bias,
                         addend=x.add, etypes=G.et32)
    _guards_ok((rb, ret))
    return ret


def _backward(G, x, want_gh=True):
    (hb, gh), (wb, gw) = _out(G.n_src, x.fi), _out(G.R, x.fi, x.fo)
    if x.lw is None:
        K.rgcn_layer1_backward(G.gidx, x.h, x.w, G.norm, x.go, gh, gw, etypes=G.et32)
        _guards_ok((hb, gh), (wb, gw))
        return gh, gw, None
    lb, gl = _out(x.fi, x.fo)
    K.rgcn_layer1_backward_ex(G.gidx, x.h, x.w, G.norm, x.lw, x.go, gh if want_gh else None,
                              gw, gl, etypes=G.et32)
    _guards_ok((wb, gw), (lb, gl))
    if not want_gh:  # untouched
        assert th.equal(hb.view(th.int32), th.full_like(hb, SENT).view(th.int32))
        return None, gw, gl
    _guards_ok((hb, gh))
    return gh, gw, gl


def _same(got, ref, what):
    for name, a, b in zip(("ret", "grad_hidden", "grad_weight", "grad_loop"), got, ref):
        assert (a is None) == (b is None), (what, name)
        if a is not None:
            assert th.equal(a, b), (what, name, int((a != b).sum()), float((a - b).abs().max()))


def _run(G, x):
    return (_forward(G, x),) + _backward(G, x)


# --------------------------------------------------------------------------- #
# which kernel a product takes
# --------------------------------------------------------------------------- #
def _gemm(m, n, k, a, b, a_al=True, b_al=True, splits=1):
    return _ffi.lib().DGLMIRgcnGemmInstance(m, n, k, a[0], a[1], b[0], b[1], int(a_al), int(b_al),
                                            splits)


def _routes(n, fi, R, fo, h_al=True):
    """The instances of the six products of the unfused entries (capi.cpp
    rgcn_layer1_impl / rgcn_layer1_backward_impl) on a square graph of n nodes; the
    library's own operands (W_cat, gy) are 16-byte aligned allocations."""
    S = _ffi.lib().DGLMIRgcnGemmSplits
    M = R * fo
    return (_gemm(n, M, fi, (fi, 1), (M, 1), h_al),
            _gemm(n, fi, M, (M, 1), (1, M)),
            _gemm(fi, M, n, (1, fi), (M, 1), h_al, True, S(fi, M, n)),
            _gemm(n, fo, fi, (fi, 1), (fo, 1), h_al),
            _gemm(n, fi, fo, (fo, 1), (1, fo)),
            _gemm(fi, fo, n, (1, fi), (fo, 1), h_al, True, S(fi, fo, n)))


def _fused_code(tile, width):
    blocks = 1 if width <= 32 else (2 if width <= 64 else 4)
    return 1600 + 2 * blocks if tile == "16" else 3200 + blocks


def _fused(G, x, rels):
    """(forward, backward) fused instance of a call, by shape."""
    F = _ffi.lib().DGLMIRgcnFusedInstance
    assert x.h.data_ptr() % 16 == 0 and x.go.data_ptr() % 16 == 0 and G.m > 0
    return F(x.fi, x.fo, rels, G.n_dst, G.n_src), F(x.fo, x.fi, rels, G.n_src, G.n_dst)


def _fused_gw(n_src, fi, rels, h_al=True):
    """The product after the fused backward walk (rgcn_layer1_backward_impl): hidden^T
    (F_in x N) . gy (N x rels * 64) -- gy holds the relation blocks and, with a self-loop,
    grad_out as its last block, so one product gives every weight gradient."""
    mg = rels * 64
    return _gemm(fi, mg, n_src, (1, fi), (mg, 1), h_al, True,
                 _ffi.lib().DGLMIRgcnGemmSplits(fi, mg, n_src))


def _tn_box(m, n, k):
    """gemm_tn_instance restated for an aligned column-major A and row-major B under
    gemm_splits' count (>= 2 from k = 1024 on): what a test expects of _fused_gw."""
    if k < 4096 or m % 4 or n % 4:
        return K_GEMM
    for code, mm, nn in ((TN_2_8, 64, 256), (TN_2_10, 64, 320), (TN_4_4, 128, 128), (TN_8_2, 256, 64)):
        if m <= mm and n <= nn:
            return code
    return K_GEMM


# --------------------------------------------------------------------------- #
# 1. the GEMM family
# --------------------------------------------------------------------------- #
# (F_in, R, F_out): (forward, grad_hidden, weight gradient), (the self-loop products)
GEMM_SHAPES = [
    ((64, 4, 64), (ROWS_8_64, ROWS_2_256, TN_2_8), (ROWS_8_64, ROWS_8_64, TN_2_8)),
    ((4, 1, 1), (ROWS_8_64, K_GEMM, K_GEMM), (ROWS_8_64, K_GEMM, K_GEMM)),
    ((60, 5, 50), (ROWS_8_64, K_GEMM, K_GEMM), (ROWS_8_64, K_GEMM, K_GEMM)),
    ((128, 2, 64), (ROWS_4_128, ROWS_4_128, TN_4_4), (ROWS_4_128, ROWS_8_64, TN_4_4)),
    ((68, 3, 11), (ROWS_4_128, K_GEMM, K_GEMM), (ROWS_4_128, K_GEMM, K_GEMM)),
    ((256, 2, 32), (ROWS_2_256, ROWS_8_64, TN_8_2), (ROWS_2_256, ROWS_8_64, TN_8_2)),
    ((132, 1, 33), (ROWS_2_256, K_GEMM, K_GEMM), (ROWS_2_256, K_GEMM, K_GEMM)),
    ((64, 5, 64), (K_GEMM, K_GEMM, TN_2_10), (ROWS_8_64, ROWS_8_64, TN_2_8)),
    ((128, 4, 64), (K_GEMM, K_GEMM, K_GEMM), (ROWS_4_128, ROWS_8_64, TN_4_4)),
    ((30, 2, 7), (K_GEMM, K_GEMM, K_GEMM), (K_GEMM, K_GEMM, K_GEMM)),
    ((260, 1, 16), (K_GEMM, K_GEMM, K_GEMM), (K_GEMM, K_GEMM, K_GEMM)),
]
GEMM_IDS = ["%d-%d-%d" % s[0] for s in GEMM_SHAPES]


def _gemm_case(n, fi, R, fo, main, loop, m=40000, offset=0, layers=2):
    G = _square(n, R, m)
    assert _routes(n, fi, R, fo, h_al=not offset) == main + loop, _routes(n, fi, R, fo, not offset)
    for with_loop in (False, True):
        x = _inputs(G, fi, fo, seed=1000 * fi + 10 * fo + R + with_loop, loop=with_loop, offset=offset)
        ref = _reference(G, x)
        _state(G, 0)
        plain = _run(G, x)
        _same(plain, ref, "stateless")
        _state(G, layers)
        prepared = _run(G, x)
        _same(prepared, ref, "prepared")
        _same(prepared, plain, "prepared against stateless")
        _state(G, 0)


@pytest.mark.parametrize("n", [4095, 4096, 4097, 4127])
@pytest.mark.parametrize("shape,main,loop", GEMM_SHAPES, ids=GEMM_IDS)
def test_gemm_family(shape, main, loop, n):
    """Every product of the unfused entries -- forward, both gradients and the self-loop
    products of the Ex entries -- stateless and with a prepared state (layers = 2), one
    node below the tall-kernel threshold (everything on k_gemm), at it, one above, and at
    N % 32 = 31 (a last row tile short of one row)."""
    if n < 4096:
        main = loop = (K_GEMM,) * 3
    _gemm_case(n, *shape, main, loop)


# N: (splits, rows per block, blocks, rows of the last block) of launch_tn
TN_TAILS = {4129: (8, 544, 8, 321), 8193: (16, 544, 16, 33), 16865: (32, 544, 32, 1),
            16896: (32, 544, 32, 32)}


@pytest.mark.parametrize("n", sorted(TN_TAILS))
@pytest.mark.parametrize("shape,main,loop", [s for s in GEMM_SHAPES if s[1][2] >= TN_2_8],
                         ids=[i for i, s in zip(GEMM_IDS, GEMM_SHAPES) if s[1][2] >= TN_2_8])
def test_gemm_tn_tails(shape, main, loop, n):
    """k_gemm_tn's last block (the derivation is in the file's docstring): N = 4129 --
    8 blocks of 544 rows (17 slices, odd), the last of 321 rows (11 slices, the last of
    one row); N = 8193 -- 16 blocks of 544, the last of 33 rows (a full slice and a
    one-row slice); N = 16865 -- 32 blocks of 544, the last of a single row (one slice,
    partial: no second load, only the tail step); N = 16896 -- the same with a last block
    of exactly one full 32-row slice."""
    fi, R, fo = shape
    sp = _ffi.lib().DGLMIRgcnGemmSplits(fi, R * fo, n)
    rpb = -(-(-(-n // min(sp, 512))) // 32) * 32
    blocks = -(-n // rpb)
    assert (sp, rpb, blocks, n - (blocks - 1) * rpb) == TN_TAILS[n]
    _gemm_case(n, fi, R, fo, main, loop, m=30000)


def test_unaligned_hidden_falls_back():
    """hidden 4 bytes into its buffer: the float4 loads of k_gemm_rows and k_gemm_tn are
    not possible, the forward and the weight gradient take k_gemm (grad_hidden reads the
    library's own gy: still rows<2,256>); with a state of layers = 6 the forward is not
    fused either, the backward is (grad_out is aligned) and its weight-gradient product
    over the unaligned hidden takes k_gemm."""
    main, loop = (K_GEMM, ROWS_2_256, K_GEMM), (K_GEMM, ROWS_8_64, K_GEMM)
    _gemm_case(4097, 64, 4, 64, main, loop, offset=1, layers=6)
    # the products behind the fused backward (64 x 256, and 64 x 320 with the self-loop):
    # tn<2,8> / tn<2,10> for an aligned hidden, k_gemm for this one
    assert (_fused_gw(4097, 64, 4), _fused_gw(4097, 64, 5)) == (TN_2_8, TN_2_10)
    assert (_fused_gw(4097, 64, 4, False), _fused_gw(4097, 64, 5, False)) == (K_GEMM, K_GEMM)


# --------------------------------------------------------------------------- #
# 2. the fused walks
# --------------------------------------------------------------------------- #
def _fused_case(G, fi, fo, tile, loop, cached, seed, want=True, gw=None):
    """One shape on the fused route (or, want = False, a shape the rule refuses): forward
    and backward with a state of layers = 4 against the reference and the unfused call;
    gw names the kernel of the weight-gradient product behind the fused backward."""
    x = _inputs(G, fi, fo, seed=seed, loop=loop)
    rels = G.R + int(loop)
    f, b = _fused(G, x, rels)
    assert f == (_fused_code(tile, fo) if want and fi == 64 else 0), (f, fi, fo, rels)
    assert b == (_fused_code(tile, fi) if want and fo == 64 else 0), (b, fi, fo, rels)
    if b:  # the weight gradients' product behind the fused backward walk
        assert _fused_gw(G.n_src, fi, rels) == _tn_box(fi, rels * 64, G.n_src), (fi, rels, G.n_src)
        if gw is not None:
            assert _fused_gw(G.n_src, fi, rels) == gw, (fi, rels, G.n_src)
    ref = _reference(G, x)
    _state(G, 0)
    plain = _run(G, x)
    _same(plain, ref, "unfused")
    _state(G, 4, cached)
    got = _run(G, x)
    _same(got, ref, "fused")
    _same(got, plain, "fused against unfused")
    if loop:  # no input gradient wanted: the same weight gradients, bit for bit
        gh2, gw2, gl2 = _backward(G, x, want_gh=False)
        assert gh2 is None and th.equal(gw2, got[2]) and th.equal(gl2, got[3])
    _state(G, 0)


WIDTHS = [1, 31, 32, 33, 64, 65, 127, 128]


@pytest.mark.parametrize("cached", [True, False], ids=["norm-streamed", "norm-by-eid"])
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("tile", ["16", "32"])
def test_fused_widths(monkeypatch, tile, width, cached):
    """Forward at F_out = width and backward at F_in = width, one column either side of
    the 32-column blocks: all six instances of each kernel, over the designed tiles.  The
    backward's weight-gradient product hidden^T . gy (width x 128 over 4129 nodes) is
    tn<2,8> at widths 32 and 64, tn<4,4> at 128 and k_gemm at the widths off a multiple
    of 4."""
    monkeypatch.setenv("DGLMI_RGCN_TILE", tile)
    G = _square(4129, 2)
    _fused_case(G, 64, width, tile, False, cached, seed=width, gw=TN_2_8)
    if width != 64:
        _fused_case(G, width, 64, tile, False, cached, seed=500 + width,
                    gw={32: TN_2_8, 128: TN_4_4}.get(width, K_GEMM))


@pytest.mark.parametrize("loop", [False, True], ids=["plain", "self-loop"])
@pytest.mark.parametrize("width,last", [(32, 10), (64, 5), (128, 2)])
@pytest.mark.parametrize("tile", ["16", "32"])
def test_fused_lds_limit(monkeypatch, tile, width, last, loop):
    """The last relation count whose matrices (with the self-loop one) fit the weights'
    20480 LDS floats for the width class, forward and backward; one more relation is not
    fused and gives the same exact results.  With a self-loop: bias and addend in the
    forward, grad_loop in the backward, and BackwardEx without grad_hidden."""
    monkeypatch.setenv("DGLMI_RGCN_TILE", tile)
    R = last - int(loop)
    for rels, want in ((R, True), (R + 1, False)):
        G = _square(1729, rels, m=20000)
        # 1729 nodes: below k_gemm_tn's 4096, the weight-gradient product is k_gemm
        _fused_case(G, 64, width, tile, loop, True, seed=width + rels, want=want, gw=K_GEMM)
        if width != 64:
            _fused_case(G, width, 64, tile, loop, True, seed=700 + width + rels, want=want,
                        gw=K_GEMM)


def _queue_tiles(n, tile):
    """Tiles per queue of the fused launch (launch_rgcn_fused and the kernels' queues)."""
    rows, waves = (16, 16) if tile == "16" else (32, 8)
    tiles = -(-n // rows)
    nq = min(8, min(256, -(-tiles // waves)))
    return [-(-(tiles - q) // nq) for q in range(nq) if tiles > q]


ROW_COUNTS = [4129, 4144, 4145, 4159, 1, 15, 16, 17, 33]


def test_fused_row_counts_meet_the_queue_edges():
    """ROW_COUNTS holds N % 32 = 1, 16, 17, 31, grids of fewer than eight queues, and a
    per-queue tile count that is no multiple of the grab size (4 tiles of 16 rows, 2 of
    32)."""
    assert {n % 32 for n in ROW_COUNTS} >= {1, 16, 17, 31}
    for tile, grab in (("16", 4), ("32", 2)):
        assert any(len(_queue_tiles(n, tile)) < 8 for n in ROW_COUNTS)
        assert len(_queue_tiles(4129, tile)) == 8
        assert any(q % grab for q in _queue_tiles(4129, tile))


@pytest.mark.parametrize("n", ROW_COUNTS)
@pytest.mark.parametrize("tile", ["16", "32"])
def test_fused_row_counts(monkeypatch, tile, n):
    """Partial last tiles and small grids, 64 -> 64 with four relations and the self-loop
    (five matrices: the LDS limit), the norm streamed or gathered by edge id in turn.  The
    weight gradients come from one product hidden^T . gy, 64 x 320: tn<2,10> from 4096
    nodes on, k_gemm on the small grids."""
    monkeypatch.setenv("DGLMI_RGCN_TILE", tile)
    G = _square(n, 4, m=30000 if n > 1000 else 30 * n + 5, seed=n)
    _fused_case(G, 64, 64, tile, True, n % 2 == 1, seed=n, gw=TN_2_10 if n >= 4096 else K_GEMM)


@pytest.mark.parametrize("n_src,n_dst", [(4129, 2065), (2065, 4129)])
@pytest.mark.parametrize("tile", ["16", "32"])
def test_fused_rectangular_block(monkeypatch, tile, n_src, n_dst):
    """num_src != num_dst, no self-loop: the forward walks num_dst rows and gathers from
    num_src, the backward the other way round."""
    monkeypatch.setenv("DGLMI_RGCN_TILE", tile)
    G = _graph(n_src, n_dst, 3, 30000, 11)
    # hidden^T . gy reduces over the sources: 64 x 192, tn<2,8> from 4096 of them on
    _fused_case(G, 64, 64, tile, False, True, seed=n_src, gw=TN_2_8 if n_src >= 4096 else K_GEMM)


# --------------------------------------------------------------------------- #
# 3. layer 0
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("F", [1, 7, 16, 64])
def test_layer0(F):
    """rgcn_layer0 / _backward (the typed gather alone) on the designed graph, stateless
    and prepared (norm streamed, and gathered by edge id), exact."""
    G = _square(4129, 3)
    gen = th.Generator(device=DEV).manual_seed(F)
    w = _ints(gen, (G.R, G.n_src, F), -2, 2)
    go = _guarded(gen, G.n_dst, F, -4, 4)
    nrm = G.norm.double()
    ref = th.zeros(G.n_dst, F, dtype=th.float64, device=DEV).index_add_(
        0, G.d, w.double()[G.et, G.s] * nrm)
    gref = th.zeros(G.R * G.n_src, F, dtype=th.float64, device=DEV).index_add_(
        0, G.et * G.n_src + G.s, go.double()[G.d] * nrm)
    mass = th.zeros(G.n_dst, F, dtype=th.float64, device=DEV).index_add_(
        0, G.d, w.double().abs()[G.et, G.s] * nrm)
    gmass = th.zeros(G.R * G.n_src, F, dtype=th.float64, device=DEV).index_add_(
        0, G.et * G.n_src + G.s, go.double().abs()[G.d] * nrm)
    assert max(float(mass.max()), float(gmass.max())) < LIMIT
    for layers, cached in ((0, True), (1, True), (1, False)):
        _state(G, layers, cached)
        (rb, ret), (wb, gw) = _out(G.n_dst, F), _out(G.R, G.n_src, F)
        K.rgcn_layer0(G.gidx, w, G.norm, ret, etypes=G.et32)
        K.rgcn_layer0_backward(G.gidx, go, G.norm, gw, etypes=G.et32)
        _guards_ok((rb, ret), (wb, gw))
        assert th.equal(ret, ref.float()), (layers, cached)
        assert th.equal(gw.view(-1, F), gref.float()), (layers, cached)
    _state(G, 0)
