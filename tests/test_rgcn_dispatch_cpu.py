"""The dispatch of the R-GCN layer-1 products and fused walks (csrc/hack_kernels.hip
gemm_splits, gemm_instance, rgcn_fused_instance -- the rules launch_gemm and
launch_rgcn_fused call) through the host queries DGLMIRgcnGemmSplits,
DGLMIRgcnGemmInstance and DGLMIRgcnFusedInstance, tabled at both sides of every
threshold in the code.  No device work: the queries are pure host functions."""
import pytest

from dgl import _ffi

GENERIC, ROWS_8_64, ROWS_4_128, ROWS_2_256, TN_2_8, TN_2_10, TN_4_4, TN_8_2 = range(8)


def inst(m, n, k, a=None, b=None, a_al=1, b_al=1, splits=1):
    """DGLMIRgcnGemmInstance; a / b = (row, column) strides, default row-major."""
    a = (k, 1) if a is None else a
    b = (n, 1) if b is None else b
    return _ffi.lib().DGLMIRgcnGemmInstance(m, n, k, a[0], a[1], b[0], b[1], a_al, b_al, splits)


def tn(m, n, k, splits=2, a_al=1, b_al=1, a=None, b=None):
    """A = hidden^T: (k x m) row-major read as (m x k) with strides (1, m)."""
    return inst(m, n, k, (1, m) if a is None else a, b, a_al, b_al, splits)


def fused(gw, ow, rels, rows=4097, t_rows=-1):
    return _ffi.lib().DGLMIRgcnFusedInstance(gw, ow, rels, rows, t_rows)


def test_gemm_splits():
    """tiles = ceil(M / 128) ceil(N / 64); doubled while tiles * splits < 4096, K / (2
    splits) >= 512 and splits < 2048."""
    S = _ffi.lib().DGLMIRgcnGemmSplits

    def model(m, n, k):
        tiles, s = -(-m // 128) * -(-n // 64), 1
        while tiles * s < 4096 and k // (s * 2) >= 512 and s < 2048:
            s *= 2
        return s
    # K at the first doubling: K / 2 >= 512
    assert S(64, 64, 1023) == 1 and S(64, 64, 1024) == 2
    assert S(64, 64, 2047) == 2 and S(64, 64, 2048) == 4
    # the node counts of tests/test_rgcn_shapes_gpu.py
    assert S(64, 256, 4095) == 4 and S(64, 256, 4096) == S(64, 256, 4097) == 8  # K / 8 >= 512
    # tiles * splits reaches 4096: 8 tiles stop at 512 splits, 1 tile at the 2048 cap
    assert S(128, 512, 1 << 30) == 512 and S(129, 512, 1 << 30) == 256
    assert S(1, 1, 1 << 30) == 2048
    # an output that fills the device is never split
    assert S(128 * 64, 64 * 64, 1 << 20) == 1 and S(128 * 64 - 128, 64 * 64, 1 << 20) == 2
    for m, n, k in [(64, 256, 4097), (128, 256, 8223), (4, 1, 4095), (60, 250, 4127), (256, 64, 6000),
                    (1, 1, 511), (300, 300, 100000)]:
        assert S(m, n, k) == model(m, n, k), (m, n, k)


def test_no_kernel_for_empty_products():
    assert inst(0, 8, 8) == -1 and inst(8, 0, 8) == -1 and inst(8, 8, 0) == -1
    assert inst(1, 1, 1) == GENERIC


def test_rows_preconditions():
    """k_gemm_rows: M >= 4096, A row-major, a_rs % 4 == 0, K % 4 == 0, A aligned."""
    assert inst(4095, 64, 64) == GENERIC and inst(4096, 64, 64) == ROWS_8_64
    assert inst(4096, 64, 63) == GENERIC and inst(4096, 64, 62) == GENERIC
    assert inst(4096, 64, 61) == GENERIC and inst(4096, 64, 60) == ROWS_8_64
    assert inst(4096, 64, 4) == ROWS_8_64 and inst(4096, 1, 4) == ROWS_8_64
    # a wider row stride: a multiple of 4 is taken, anything else is not
    assert inst(4096, 64, 60, a=(64, 1)) == ROWS_8_64
    for rs in (61, 62, 63):
        assert inst(4096, 64, 60, a=(rs, 1)) == GENERIC
    assert inst(4096, 64, 64, a_al=0) == GENERIC
    assert inst(4096, 64, 64, b_al=0) == ROWS_8_64   # B is read by scalars
    assert inst(4096, 64, 64, a=(1, 4096)) == GENERIC  # column-major A
    # B's strides do not matter (grad_hidden reads W_cat^T)
    assert inst(4096, 64, 256, b=(1, 256)) == ROWS_2_256
    # the split count does not matter, and rows comes before tn
    assert inst(4096, 64, 64, splits=8) == ROWS_8_64


def test_rows_boxes():
    """<8,64>: N <= 256, K <= 64; <4,128>: N <= 128, K <= 128; <2,256>: N <= 64, K <= 256;
    the first that fits."""
    m = 4096
    assert inst(m, 256, 64) == ROWS_8_64 and inst(m, 257, 64) == GENERIC
    assert inst(m, 256, 68) == GENERIC and inst(m, 128, 68) == ROWS_4_128
    assert inst(m, 128, 64) == ROWS_8_64  # both fit: the first
    assert inst(m, 128, 128) == ROWS_4_128 and inst(m, 129, 128) == GENERIC
    assert inst(m, 129, 64) == ROWS_8_64
    assert inst(m, 128, 132) == GENERIC and inst(m, 64, 132) == ROWS_2_256
    assert inst(m, 64, 256) == ROWS_2_256 and inst(m, 65, 256) == GENERIC
    assert inst(m, 64, 260) == GENERIC and inst(m, 1, 260) == GENERIC
    assert inst(m, 1, 256) == ROWS_2_256


def test_tn_preconditions():
    """k_gemm_tn: K >= 4096, splits >= 2, a_rs == 1, b_cs == 1, M, N, a_cs, b_rs % 4 == 0,
    A and B aligned."""
    assert tn(64, 256, 4095) == GENERIC and tn(64, 256, 4096) == TN_2_8
    assert tn(64, 256, 4096, splits=1) == GENERIC and tn(64, 256, 4096, splits=2) == TN_2_8
    assert tn(64, 256, 4096, a_al=0) == GENERIC and tn(64, 256, 4096, b_al=0) == GENERIC
    for d in (1, 2, 3):
        assert tn(64 - d, 256, 4096) == GENERIC          # M % 4 (and with it a_cs)
        assert tn(64, 256 - d, 4096) == GENERIC          # N % 4 (and with it b_rs)
        assert tn(60, 256, 4096, a=(1, 60 + d)) == GENERIC   # a_cs % 4 alone
        assert tn(64, 252, 4096, b=(252 + d, 1)) == GENERIC  # b_rs % 4 alone
    assert tn(60, 252, 4096) == TN_2_8 and tn(4, 4, 4096) == TN_2_8
    assert tn(60, 252, 4096, a=(1, 64), b=(256, 1)) == TN_2_8
    assert tn(64, 256, 4096, a=(64, 1)) == GENERIC           # A not transposed, M < 4096
    assert tn(64, 256, 4096, b=(1, 4096)) == GENERIC         # B column-major


def test_tn_boxes():
    """<2,8>: M <= 64, N <= 256; <2,10>: M <= 64, N <= 320; <4,4>: M, N <= 128; <8,2>:
    M <= 256, N <= 64."""
    k = 4096
    assert tn(64, 256, k) == TN_2_8 and tn(64, 260, k) == TN_2_10
    assert tn(64, 320, k) == TN_2_10 and tn(64, 324, k) == GENERIC
    assert tn(68, 256, k) == GENERIC and tn(68, 132, k) == GENERIC
    assert tn(68, 128, k) == TN_4_4 and tn(128, 128, k) == TN_4_4
    assert tn(64, 128, k) == TN_2_8  # the first that fits
    assert tn(132, 128, k) == GENERIC and tn(132, 64, k) == TN_8_2
    assert tn(128, 132, k) == GENERIC
    assert tn(256, 64, k) == TN_8_2 and tn(256, 68, k) == GENERIC
    assert tn(260, 64, k) == GENERIC and tn(260, 4, k) == GENERIC
    assert tn(128, 64, k) == TN_4_4


def test_layer1_routes_of_the_flagship_shape():
    """64 -> 64, four relations, 4096 nodes: the three products of the unfused entries
    as capi.cpp issues them."""
    n, fi, r, fo = 4096, 64, 4, 64
    m = r * fo
    assert inst(n, m, fi) == ROWS_8_64
    assert inst(n, fi, m, a=(m, 1), b=(1, m)) == ROWS_2_256
    sp = _ffi.lib().DGLMIRgcnGemmSplits(fi, m, n)
    assert sp == 8 and inst(fi, m, n, a=(1, fi), b=(m, 1), splits=sp) == TN_2_8


def test_split_k_ranges_of_k_gemm():
    """(128, 4, 64) at 4097 nodes: the weight gradient (128 x 256 over N) fits no k_gemm_tn
    box; k_gemm splits N into ceil(N / ks) ranges, ks = ceil(N / splits) rounded up to 32."""
    n = 4097
    sp = _ffi.lib().DGLMIRgcnGemmSplits(128, 256, n)
    ks = -(-(-(-n // sp)) // 32) * 32
    assert sp == 8 and ks == 544 and -(-n // ks) == 8
    assert inst(128, 256, n, a=(1, 128), b=(256, 1), splits=sp) == GENERIC


def test_fused_widths(monkeypatch):
    monkeypatch.delenv("DGLMI_RGCN_TILE", raising=False)
    got = [fused(64, w, 1) for w in (0, 1, 32, 33, 64, 65, 128, 129)]
    assert got == [0, 1602, 1602, 1604, 1604, 1608, 1608, 0]
    monkeypatch.setenv("DGLMI_RGCN_TILE", "32")
    got = [fused(64, w, 1) for w in (0, 1, 32, 33, 64, 65, 128, 129)]
    assert got == [0, 3201, 3201, 3202, 3202, 3204, 3204, 0]
    monkeypatch.setenv("DGLMI_RGCN_TILE", "16")
    assert fused(64, 64, 4) == 1604
    monkeypatch.setenv("DGLMI_RGCN_TILE", "8")  # anything but 32 is 16
    assert fused(64, 64, 4) == 1604


@pytest.mark.parametrize("tile", ["16", "32"])
def test_fused_lds_bound(monkeypatch, tile):
    """R * 64 * nb * 32 <= 20480 floats, R counting the self-loop matrix: 10 / 5 / 2
    matrices at widths <= 32 / <= 64 / <= 128."""
    monkeypatch.setenv("DGLMI_RGCN_TILE", tile)
    for lo, hi, last in [(1, 32, 10), (33, 64, 5), (65, 128, 2)]:
        for w in (lo, hi):
            assert 64 * last * (-(-w // 32) if w <= 64 else 4) * 32 <= 20480
            assert fused(64, w, last) != 0 and fused(64, w, last + 1) == 0, (w, last)
            assert fused(64, w, 1) == fused(64, w, last)
    assert fused(64, 64, 0) == 0 and fused(64, 64, -1) == 0


def test_fused_gathered_width_and_rows(monkeypatch):
    monkeypatch.delenv("DGLMI_RGCN_TILE", raising=False)
    for gw in (0, 32, 63, 65, 128):
        assert fused(gw, 64, 2) == 0
    assert fused(64, 64, 2, rows=0) == 0 and fused(64, 64, 2, rows=1) == 1604
    # the 4 GiB rule of the 16-row kernel's 32-bit offsets: (rows + 1) * 256 and t_rows *
    # 256 bytes below 2^32, else the 32-row kernel
    lim = (1 << 32) // 256
    assert fused(64, 64, 2, rows=lim - 2) == 1604 and fused(64, 64, 2, rows=lim - 1) == 3202
    assert fused(64, 64, 2, rows=100, t_rows=lim - 1) == 1604
    assert fused(64, 64, 2, rows=100, t_rows=lim) == 3202
    assert fused(64, 128, 2, rows=100, t_rows=lim) == 3204
    # t_rows < 0 stands for num_rows
    assert fused(64, 64, 2, rows=lim - 1, t_rows=5) == 3202


def test_python_rule_agrees():
    """dgl.kernel.rgcn_fused_ok (the module's route) restates the shape rule."""
    from dgl import kernel as K
    for w in (0, 1, 32, 33, 64, 65, 128, 129):
        for r in (1, 2, 3, 5, 6, 10, 11):
            assert K.rgcn_fused_ok(64, w, r) == (fused(64, w, r) != 0), (w, r)
