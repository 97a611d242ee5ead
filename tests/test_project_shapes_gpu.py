"""DGLMIProject (csrc/kernels_project.hip: k_project, k_project_tile, k_project_glds) at
the row counts, instances, LDS images and staging paths where it can go wrong.

Every case calls the C entry on buffers the test owns: X is the first M rows of an
(M + 16, K) buffer whose 16 tail rows are NaN, Y the first M rows of an (M + 16, N)
buffer pre-filled with a sentinel.  After the call the tail rows are still the sentinel
bit for bit, no element of the first M rows is, and |y - ref| <= 2e-6 (|x| @ |w|) + 1e-6
against the fp64 product (the bound of test_nn_gpu.py::test_project_tile_kernel); NaN and
inf of the reference are matched elementwise.  A test that sets a DGLMI_PROJECT_*
variable (read by the library on every call) asserts through DGLMIProjectInstance that
the instance it meant is the one selected.
"""
import ctypes

import pytest
import torch as th

from dgl import _ffi
from dgl import backend as B
from dgl import kernel as K
from dgl._ffi import DGLError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 16            # guard rows behind X (NaN) and Y (sentinel)
SENT = -12345.0     # no product of the unit-scale draws below comes near it

# kernels_project.hip kTileCfgs: (KB, CB, NS); padded K kp = (4 / NS) 16 KB, slice width
# nsl = NS 16 CB
TILES = [(1, 4, 4), (2, 4, 4), (4, 4, 4), (4, 10, 4), (4, 4, 2), (8, 4, 2), (16, 1, 4), (8, 4, 1),
         (40, 1, 4), (4, 4, 1), (10, 4, 1), (4, 5, 4)]
KP = [(4 // ns) * 16 * kb for kb, cb, ns in TILES]
NSL = [ns * 16 * cb for kb, cb, ns in TILES]
assert KP == [16, 32, 64, 64, 128, 256, 256, 512, 640, 256, 640, 64]
assert NSL == [256, 256, 256, 640, 128, 128, 64, 64, 64, 64, 64, 320]

M_SMALL = 16 * 9 + 5


def _select(mp, k, n, cfg=None, glds=None, tile=None, expect=None):
    """Set the library's three A/B variables (None: unset) and check which kernel
    DGLMIProject will launch for (k, n): `expect` (default: the forced instance)."""
    for name, v in (("DGLMI_PROJECT_CFG", cfg), ("DGLMI_PROJECT_GLDS", glds), ("DGLMI_PROJECT_TILE", tile)):
        if v is None:
            mp.delenv(name, raising=False)
        else:
            mp.setenv(name, str(v))
    got = _ffi.lib().DGLMIProjectInstance(k, n)
    assert got == (cfg if expect is None else expect), (k, n, cfg, got)


def _groups(i, k, n, glds):
    """Workgroups per column slice of the tile launch (launch_tile_raw / launch_glds)."""
    kb, cb, _ = TILES[i]
    slices = -(-n // NSL[i])
    occ = 1 if (k % 4 != 0 and glds) else (2 if 4 * kb * cb <= 80 else 1)
    return max(1, 256 * occ // slices)


def _deep_rows(i, k, n, glds):
    """A row count with at least four tiles per workgroup, one more tile for some, and a
    partial last tile: the two (register-staged) or three (LDS-DMA) buffers wrap."""
    return 16 * (4 * _groups(i, k, n, glds) + 1) + 5


def _call(xb, m, w, bias, yb):
    k, n = xb.shape[1], w.shape[1]
    return _ffi.lib().DGLMIProject(
        ctypes.c_void_p(xb.data_ptr()), ctypes.c_int64(m), ctypes.c_int64(k),
        ctypes.c_void_p(w.data_ptr()), ctypes.c_int64(w.shape[0]), ctypes.c_int64(w.stride(0)),
        ctypes.c_int64(w.stride(1)), ctypes.c_int64(n),
        ctypes.c_void_p(bias.data_ptr() if bias is not None else None),
        ctypes.c_void_p(yb.data_ptr()), 0, K._stream(yb))


def _sentinel(rows, n):
    return th.full((rows, n), SENT, device=DEV)


class _X:
    """X = the first m rows of an (m + PAD, k) buffer with NaN tail rows; its fp64 copy
    and magnitude are made once and shared by every weight run against it."""

    def __init__(self, m, k, gen, poison=None):
        self.m, self.k = m, k
        self.buf = th.randn(m + PAD, k, device=DEV, generator=gen)
        self.buf[m:] = float("nan")
        if poison is not None:
            poison(self.buf[:m])
        assert self.buf.is_contiguous() and self.buf.data_ptr() % 16 == 0
        self.x64 = self.buf[:m].double()
        self.a64 = self.x64.abs()


def _weight(k, n, gen):
    """(k, n) unit-scale weight with no exact zero, and a bias."""
    w = th.randn(k, n, device=DEV, generator=gen)
    w = th.where(w.abs() < 1e-3, th.full_like(w, 0.5), w)
    return w, th.randn(n, device=DEV, generator=gen)


def _check(X, w, b, biases=(False, True)):
    """Run DGLMIProject on X and the (possibly strided) weight view w, without and with
    the bias b, into a sentinel-filled Y; returns the fp64 reference (without bias)."""
    m, n = X.m, w.shape[1]
    ref = X.x64 @ w.double()
    mag = X.a64 @ w.double().abs()
    for with_bias in biases:
        bias = b if with_bias else None
        yb = _sentinel(m + PAD, n)
        rc = _call(X.buf, m, w, bias, yb)
        assert rc == 0, _ffi.last_error()
        y = yb[:m]
        tag = (m, X.k, n, with_bias)
        # nothing past row m, nothing left unwritten
        assert th.equal(yb[m:].view(th.int32), _sentinel(PAD, n).view(th.int32)), tag
        assert bool((y != SENT).all()), tag
        r = ref if bias is None else ref + bias.double()
        assert th.equal(th.isnan(y), th.isnan(r)), tag
        inf = th.isinf(r)
        assert th.equal(th.isinf(y), inf), tag
        assert th.equal(y[inf].double(), r[inf]), tag
        fin = th.isfinite(r)
        err = th.where(fin, (y.double() - r).abs() - (2e-6 * mag + 1e-6), th.zeros_like(r))
        excess = float(err.max())
        print("project m=%d k=%d n=%d bias=%d: max excess over the bound %.3e" % (tag + (excess,)))
        assert excess <= 0.0, tag
    return ref


# --------------------------------------------------------------------------- #
# 1. every instance x LDS image x staging path
# --------------------------------------------------------------------------- #
IMAGES = [("raw0", 0, None), ("raw2-glds", 2, "1"), ("raw2-regs", 2, "0"), ("raw1-glds", 1, "1"),
          ("raw1-regs", 1, "0")]


@pytest.mark.parametrize("image,dk,glds", IMAGES, ids=[im[0] for im in IMAGES])
@pytest.mark.parametrize("inst", range(12))
def test_instance_image_staging(monkeypatch, inst, image, dk, glds):
    """Instance `inst` forced, K = kp (padded image) / kp - 2 (K even, the span itself) /
    kp - 1 (K odd), the latter two through the LDS-DMA kernel and the register-staged
    one; N = nsl, nsl - 1, nsl - 2 (float4, scalar and float2 stores) and nsl + 3 (a
    second, almost empty slice), with and without bias; a few tiles and a launch deep
    enough that every workgroup wraps its LDS buffers."""
    k = KP[inst] - dk
    gen = th.Generator(device=DEV).manual_seed(100 * inst + dk)
    ns = [NSL[inst], NSL[inst] - 1, NSL[inst] - 2, NSL[inst] + 3]
    deep = sorted({_deep_rows(inst, k, n, glds != "0") for n in ns})
    xs = {m: _X(m, k, gen) for m in [M_SMALL] + deep}
    for n in ns:
        _select(monkeypatch, k, n, cfg=inst, glds=glds, tile="1")
        w, b = _weight(k, n, gen)
        for m in (M_SMALL, _deep_rows(inst, k, n, glds != "0")):
            _check(xs[m], w, b)


# --------------------------------------------------------------------------- #
# 2. short and padded K
# --------------------------------------------------------------------------- #
def _short_ks(inst):
    kb, _, ns = TILES[inst]
    kp, kw, ks = KP[inst], 16 * kb, 4 // ns
    out = {kp - 12}                       # K % 4 == 0 below kp: the zero-padded columns
    if kp >= 32:
        out |= {kp - 17, kp - 18, kp - 20}  # a whole 16-k block past K, in each image
    if ks == 4:
        out |= {kw + 10, kw + 9, kw + 2, kw + 4}  # instance 10: 170, 169, 162: two waves' k past K
    if ks == 2:
        out |= {kw - 6, kw - 7, kw - 4}     # the second wave's k past K
    if inst == 0:
        out |= {1, 2, 3, 4}
    assert all(0 < k <= kp for k in out)
    return sorted(out)


@pytest.mark.parametrize("inst", range(12))
def test_short_and_padded_k(monkeypatch, inst):
    """K well below the instance's padded K: a whole 16-k block, and with a k split a
    whole wave's k-slice, past K (zero W rows against masked or zero-padded X), in the
    padded image and in both RAW images on both staging paths; instance 0 down to K = 1;
    N = 1 once."""
    gen = th.Generator(device=DEV).manual_seed(7000 + inst)
    n = NSL[inst] - 1
    for k in _short_ks(inst):
        m_deep = 16 * 1030 + 4
        xs = [_X(M_SMALL, k, gen), _X(m_deep, k, gen)]
        w, b = _weight(k, n, gen)
        for glds in ([None] if k % 4 == 0 else ["1", "0"]):
            _select(monkeypatch, k, n, cfg=inst, glds=glds, tile="1")
            for X in xs:
                _check(X, w, b)
            if inst == 0 and k == 3:
                w1, b1 = _weight(k, 1, gen)
                _select(monkeypatch, k, 1, cfg=inst, glds=glds, tile="1")
                _check(xs[0], w1, b1)


# --------------------------------------------------------------------------- #
# 3. row-count sweep, 5. non-finite containment: one (K, N) per image and staging path
# --------------------------------------------------------------------------- #
ROWS = [16, 17, 31, 32, 33, 47, 48, 64, 16 * 256, 16 * 256 + 1, 16 * 257 + 8, 16 * 512, 16 * 513 + 4,
        16 * 2049, 16 * 2049 + 5, 16 * 2049 + 8]
# (id, k, n, cfg, glds, tile, expected instance)
PATHS = [("i10-raw0", 600, 64, 10, None, None, 10),
         ("i10-raw2-glds", 602, 64, 10, "1", None, 10),
         ("i10-raw2-regs", 602, 64, 10, "0", None, 10),
         ("i10-raw1-glds", 601, 64, 10, "1", None, 10),
         ("i10-raw1-regs", 601, 64, 10, "0", None, 10),
         ("i2-raw1-glds", 63, 130, 2, "1", None, 2),
         ("i2-raw1-regs", 63, 130, 2, "0", None, 2),
         ("i2-raw2-glds", 62, 130, 2, "1", None, 2),
         ("i2-raw2-regs", 62, 130, 2, "0", None, 2),
         ("direct-64x64", 64, 64, None, None, None, -2),
         ("direct-128x128", 128, 128, None, None, None, -2),
         ("tile-64x128", 64, 128, None, None, "1", 2)]
PATH_IDS = [p[0] for p in PATHS]


def test_row_sweep_meets_both_tail_branches():
    """k_project_glds copies the tile holding X's end 16 bytes at a time clamped to the
    last aligned float4 when M K % 4 == 0, 4 bytes at a time otherwise; k_project_tile's
    load_part runs when M % 16 != 0.  ROWS meets, for every RAW K of PATHS: a partial
    last tile with M K % 4 == 0, one with M K % 4 != 0, and a whole last tile; and tile
    counts below, at and above the group counts (256 and 512)."""
    for _, k, _, _, _, _, _ in PATHS:
        if k % 4 == 0:
            continue
        assert any((m * k) % 4 == 0 and m % 16 != 0 for m in ROWS), k
        assert any((m * k) % 4 != 0 for m in ROWS), k
    assert any(m % 16 == 0 for m in ROWS)
    tiles = {-(-m // 16) for m in ROWS}
    assert 1 in tiles and 2 in tiles and min(ROWS) == 16
    for g in (256, 512):
        assert g in tiles and any(g < t <= g + 2 for t in tiles)
        assert any(1 < t < g for t in tiles) and any(t > 4 * g for t in tiles)


@pytest.mark.parametrize("path,k,n,cfg,glds,tile,expect", PATHS, ids=PATH_IDS)
def test_row_sweep(monkeypatch, path, k, n, cfg, glds, tile, expect):
    """Every row count of ROWS -- one tile, fewer tiles than workgroups, whole and partial
    last tiles of both copy forms, deep launches -- on each kernel path."""
    _select(monkeypatch, k, n, cfg=cfg, glds=glds, tile=tile, expect=expect)
    gen = th.Generator(device=DEV).manual_seed(31 * k + n)
    w, b = _weight(k, n, gen)
    for m in ROWS:
        _check(_X(m, k, gen), w, b, biases=(m % 2 == 0,))
    _check(_X(ROWS[-2], k, gen), w, b)


def _poison(m):
    """Non-finite rows with clean neighbours on both sides (row indices for m rows)."""
    part = 16 * (m // 16)               # first row of the partial last tile
    assert m % 16 >= 5 and m >= 96
    rows = {"nan_row": 16 * 2 + 7,      # all NaN, in the middle of a tile
            "inf_last": 16 * 3 + 2,     # +inf at column K - 1
            "nan_first": 16 * 4 + 9,    # NaN at column 0
            "nan_part": part,           # all NaN, first row of the partial tile
            "nan_end": m - 1}           # all NaN, the last row
    picked = sorted(rows.values())
    assert all(b - a >= 2 for a, b in zip(picked, picked[1:])) and picked[0] >= 1

    def plant(x):
        x[rows["nan_row"]] = float("nan")
        x[rows["inf_last"], -1] = float("inf")
        x[rows["nan_first"], 0] = float("nan")
        x[rows["nan_part"]] = float("nan")
        x[rows["nan_end"]] = float("nan")
    return rows, plant


@pytest.mark.parametrize("path,k,n,cfg,glds,tile,expect", PATHS, ids=PATH_IDS)
def test_non_finite_rows_stay_contained(monkeypatch, path, k, n, cfg, glds, tile, expect):
    """A NaN / inf in X reaches exactly the outputs of its own row: the k-block that
    straddles K in the RAW images holds the next row's first floats (W is zero there, so
    only a non-finite neighbour shows a missing mask), and rows past M of the last tile
    are computed and dropped."""
    _select(monkeypatch, k, n, cfg=cfg, glds=glds, tile=tile, expect=expect)
    gen = th.Generator(device=DEV).manual_seed(77 * k + n)
    w, b = _weight(k, n, gen)
    assert bool((w != 0).all())
    for m in (M_SMALL, 16 * 2049 + 5):
        rows, plant = _poison(m)
        X = _X(m, k, gen, poison=plant)
        ref = _check(X, w, b)
        # the reference itself: NaN in the planted rows only, +-inf by W's last row
        nan_rows = th.zeros(m, dtype=th.bool, device=DEV)
        nan_rows[[rows["nan_row"], rows["nan_first"], rows["nan_part"], rows["nan_end"]]] = True
        assert th.equal(th.isnan(ref), nan_rows[:, None].expand(m, n))
        inf_rows = th.zeros(m, dtype=th.bool, device=DEV)
        inf_rows[rows["inf_last"]] = True
        assert th.equal(th.isinf(ref), inf_rows[:, None].expand(m, n))
        assert th.equal(th.sign(ref[rows["inf_last"]]), th.sign(w[-1].double()))


# --------------------------------------------------------------------------- #
# 4. refusals
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("k,n,inst", [(64, 64, -2), (602, 64, 10), (63, 130, 2)])
def test_short_row_counts_refused(monkeypatch, k, n, inst):
    """m = 1 and 15 (below one tile) are refused with Y untouched; m = 0 returns
    without writing."""
    _select(monkeypatch, k, n, expect=inst)
    gen = th.Generator(device=DEV).manual_seed(5)
    X = _X(16, k, gen)
    w, b = _weight(k, n, gen)
    for m in (1, 15):
        yb = _sentinel(16 + PAD, n)
        assert _call(X.buf, m, w, b, yb) != 0
        with pytest.raises(DGLError, match="m >= 16"):
            _ffi.check_call(_call(X.buf, m, w, b, yb))
        assert th.equal(yb.view(th.int32), _sentinel(16 + PAD, n).view(th.int32))
    yb = _sentinel(16 + PAD, n)
    assert _call(X.buf, 0, w, b, yb) == 0
    assert th.equal(yb.view(th.int32), _sentinel(16 + PAD, n).view(th.int32))


# --------------------------------------------------------------------------- #
# 6. weight views
# --------------------------------------------------------------------------- #
def _views(k, n, gen):
    a = th.randn(k, n + 9, device=DEV, generator=gen)
    bt = th.randn(n, k + 6, device=DEV, generator=gen)
    c = th.randn(2 * k, 3 * n, device=DEV, generator=gen)
    return [("cols", a, lambda t: t[:, 5:5 + n]),
            ("t-rows", bt, lambda t: t.t()[3:3 + k]),
            ("steps", c, lambda t: t[::2, ::3])]


@pytest.mark.parametrize("view", ["cols", "t-rows", "steps"])
@pytest.mark.parametrize("k,n,inst", [(64, 64, -2), (64, 100, 2), (602, 64, 10), (602, 100, 10)])
def test_weight_views(monkeypatch, k, n, inst, view):
    """Slices of a wider parameter -- a base pointer off 16-byte alignment, row and
    column strides other than (n, 1) and (1, k) -- take the same kernels: the C entry,
    K.project_mfma and B.project's forward and dX against fp64."""
    _select(monkeypatch, k, n, expect=inst)
    gen = th.Generator(device=DEV).manual_seed(13 * k + n)
    m = K.PROJECT_MIN_ROWS + 8
    big, cut = [(t, f) for name, t, f in _views(k, n, gen) if name == view][0]
    w = cut(big)
    assert w.shape == (k, n) and not w.is_contiguous()
    if view == "cols":
        assert w.data_ptr() % 16 != 0
    X = _X(m, k, gen)
    x = X.buf[:m]
    b = th.randn(n, device=DEV, generator=gen)
    assert K.project_mfma_ok(x, w) and K.project_mfma_ok(th.empty(m, n, device=DEV), w.t())
    ref = _check(X, w, b)
    mag = X.a64 @ w.double().abs()
    for bias in (None, b):
        r = ref if bias is None else ref + bias.double()
        y = K.project_mfma(x, w, bias)
        assert bool(((y.double() - r).abs() <= 2e-6 * mag + 1e-6).all())
    # B.project on the view of a leaf parameter: forward, and dX = dY W^T on the kernel
    leaf = big.clone().requires_grad_()
    xr = x.clone().requires_grad_()
    gy = th.randn(m, n, device=DEV, generator=gen)
    yv = B.project(xr, cut(leaf), b)
    assert bool(((yv.double() - (ref + b.double())).abs() <= 2e-6 * mag + 1e-6).all())
    yv.backward(gy)
    gref = gy.double() @ w.double().t()
    gmag = gy.double().abs() @ w.double().abs().t()
    gerr = (xr.grad.double() - gref).abs() - (2e-6 * gmag + 1e-6)
    assert float(gerr.max()) <= 0.0
