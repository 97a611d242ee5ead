"""Host-side logic of the product (no GPU): C ABI exports, shape inference,
host graph ingestion, graph bookkeeping and error behaviour."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch as th

import dgl
import dgl.function as fn
from dgl import _ffi
from dgl.graph_index import GraphIndex, host_coo_to_csr, host_csr_transpose
from oracle import oracle as O
from graphs import er_graph, g20, powerlaw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "spmat_kat.json")))


def test_library_exports_header_symbols():
    hdr = open(os.path.join(ROOT, "include", "dglmi.h")).read()
    declared = set(re.findall(r"\b(DGLMI[A-Za-z0-9]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    lib = ctypes.CDLL(_ffi._lib_path())
    for name in declared:
        assert hasattr(lib, name), name
    assert declared == set(_ffi.EXPORTED)
    assert _ffi.lib().DGLMIVersion() == b"0.4-mi355x"


@pytest.mark.parametrize("op", ["add", "sub", "mul", "div", "dot"])
def test_infer_shape_matches_oracle(op):
    rng = np.random.default_rng(0)
    shapes = [((7, 5, 3, 4), (9, 3, 1)), ((7, 4), (9, 5, 3, 4)), ((7, 5, 1, 4), (9, 5, 3, 4)),
              ((7, 1), (9, 6)), ((7, 2, 3), (9, 2, 3))]
    for a, b in shapes:
        if op == "dot" and a[-1] != b[-1]:
            continue
        x, y = th.zeros(a), th.zeros(b)
        assert dgl.kernel.infer_binary_feature_shape(op, x, y) == \
            O.infer_binary_feature_shape(op, x.numpy(), y.numpy())


def test_infer_shape_error():
    with pytest.raises(dgl.DGLError, match="Invalid broadcasting"):
        dgl.kernel.infer_binary_feature_shape("add", th.zeros(3, 5), th.zeros(3, 4))


def test_host_ingest_kat():
    for coo, csr in (("COO1", "CSR1"), ("COO2", "CSR2")):
        p, i, d = host_coo_to_csr(4, KAT[coo]["row"], KAT[coo]["col"])
        assert p.tolist() == KAT[csr]["indptr"]
        assert i.tolist() == KAT[csr]["indices"]
        assert d.tolist() == KAT[csr]["data"]
    c = KAT["CSR2"]
    p, i, d = host_csr_transpose(4, 5, c["indptr"], c["indices"], c["data"])
    assert p.tolist() == KAT["CSR2_T"]["indptr"]
    assert i.tolist() == KAT["CSR2_T"]["indices"]
    assert d.tolist() == KAT["CSR2_T"]["data"]


@pytest.mark.parametrize("maker", [g20, er_graph, lambda: powerlaw(5000, 60000, seed=2)])
def test_graph_csr_matches_oracle(maker):
    src, dst, n = maker()
    gi = GraphIndex(n)
    gi.add_edges(src, dst)
    (op, oi, od), (ip, ii, idd) = gi.host_csr()
    ref = O.RefGraph(src, dst, n)
    for a, b in zip((op, oi, od, ip, ii, idd), ref.out_csr + ref.in_csr):
        np.testing.assert_array_equal(a, b)


def test_ingest_rejects_bad_ids():
    with pytest.raises(dgl.DGLError):
        host_coo_to_csr(2, [0, 5], [0, 1])


def test_dglgraph_bookkeeping():
    g = dgl.DGLGraph()
    g.add_nodes(4)
    g.add_edges([0, 1, 2], [1, 2, 3])
    g.add_edge(3, 0)
    assert g.number_of_nodes() == 4 and g.number_of_edges() == 4
    assert g.in_degrees().tolist() == [1, 1, 1, 1]
    s, d = g.edges()
    assert s.tolist() == [0, 1, 2, 3] and d.tolist() == [1, 2, 3, 0]
    g.ndata["h"] = th.ones(4, 2)
    lv = g.local_var()
    lv.ndata["x"] = th.zeros(4, 1)
    assert "x" not in g.ndata and "h" in lv.ndata
    with pytest.raises(dgl.DGLError):
        g.ndata["bad"] = th.ones(3, 2)
    g.add_nodes(1)
    assert g.ndata["h"].shape == (5, 2)


def test_networkx_and_scipy_construction():
    import networkx as nx
    import scipy.sparse as sp
    g = dgl.DGLGraph(nx.path_graph(3))
    assert g.number_of_edges() == 4
    m = sp.coo_matrix((np.ones(3), ([0, 1, 2], [1, 2, 0])), shape=(3, 3))
    g2 = dgl.DGLGraph(m)
    assert g2.edges()[0].tolist() == [0, 1, 2]


def test_cpu_tensors_fail_loudly():
    g = dgl.DGLGraph()
    g.add_nodes(3)
    g.add_edges([0, 1], [1, 2])
    g.ndata["h"] = th.ones(3, 4)
    with pytest.raises(dgl.DGLError, match="ROCm"):
        g.update_all(fn.copy_u("h", "m"), fn.sum("m", "s"))


def test_udf_reduce_still_runs_builtin_messages_on_device():
    """A reduce UDF (degree bucketing) materialises builtin messages with the HIP
    kernel first: CPU tensors fail loudly there, no CPU fallback."""
    g = dgl.DGLGraph()
    g.add_nodes(2)
    g.add_edges([0], [1])
    g.ndata["h"] = th.zeros(2, 4)
    with pytest.raises(dgl.DGLError):
        g.update_all(fn.copy_u("h", "m"), lambda nodes: {"o": nodes.mailbox["m"].sum(1)})
    with pytest.raises(dgl.DGLError):  # a list must hold builtins only
        g.update_all(fn.copy_u("h", "m"), [fn.sum("m", "o"), lambda nodes: {}])


def test_capi_errors_without_device():
    """Reducer / op validation happens before any device work (binary_reduce_impl.h:95-98)."""
    L = _ffi.lib()
    g = _ffi.Graph()
    g.num_bits = 32
    a = _ffi.Array()
    rc = L.DGLMIKernelCopyReduce(b"mean", ctypes.byref(g), 0, ctypes.byref(a), ctypes.byref(a),
                                 None, None, None)
    assert rc == -1 and "reduce mean is not supported" in _ffi.last_error()
    rc = L.DGLMIKernelBinaryOpReduce(b"sum", b"pow", ctypes.byref(g), 0, 2, ctypes.byref(a),
                                     ctypes.byref(a), ctypes.byref(a), None, None, None, None)
    assert rc == -1 and "Unsupported binary op" in _ffi.last_error()
    g.num_bits = 16
    rc = L.DGLMIKernelCopyReduce(b"sum", ctypes.byref(g), 0, ctypes.byref(a), ctypes.byref(a),
                                 None, None, None)
    assert rc == -1 and "idx bits" in _ffi.last_error()
    # 64-bit graphs: mappings, and the int32-only entries, are refused before any device work
    g.num_bits = 64
    m = (ctypes.c_int32 * 2)()
    rc = L.DGLMIKernelCopyReduce(b"sum", ctypes.byref(g), 0, ctypes.byref(a), ctypes.byref(a),
                                 m, None, None)
    assert rc == -1 and "mappings need a graph of fewer than 2^31 edges" in _ffi.last_error()
    rc = L.DGLMIFusedGatForward(ctypes.byref(g), ctypes.byref(a), ctypes.byref(a), ctypes.byref(a),
                                0.2, ctypes.byref(a), ctypes.byref(a), ctypes.byref(a), None)
    assert rc == -1 and "fused GAT needs a graph of fewer than 2^31 edges" in _ffi.last_error()
    st = _ffi.RgcnState()
    rc = L.DGLMIRgcnPrepare(ctypes.byref(g), None, 2, 1, ctypes.byref(st), None)
    assert rc == -1 and "R-GCN needs a graph of fewer than 2^31 edges" in _ffi.last_error()


def test_builtin_names():
    assert fn.copy_src("a", "b").name == "copy_u"
    assert fn.copy_edge("a", "b").name == "copy_e"
    assert fn.src_mul_edge("a", "b", "c").name == "u_mul_e"
    assert fn.e_dot_v("a", "b", "c").name == "e_dot_v"
    assert fn.mean("m", "h").name == "mean"
    for lhs in "uve":
        for rhs in "uve":
            if lhs != rhs:
                for op in ["add", "sub", "mul", "div", "dot"]:
                    assert hasattr(fn, "%s_%s_%s" % (lhs, op, rhs))


def test_ctypes_structs_match_header_layout(tmp_path):
    """The ctypes mirrors in dgl/_ffi.py have the C layout of include/dglmi.h
    (sizes and field offsets, compiled with gcc here)."""
    import ctypes
    import os
    import subprocess
    from dgl import _ffi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = {"DGLMICsr": (_ffi.CSR, [f[0] for f in _ffi.CSR._fields_]),
              "DGLMIGraph": (_ffi.Graph, [f[0] for f in _ffi.Graph._fields_]),
              "DGLMIArray": (_ffi.Array, [f[0] for f in _ffi.Array._fields_]),
              "DGLMIEpilogue": (_ffi.Epilogue, [f[0] for f in _ffi.Epilogue._fields_]),
              "DGLMIRgcnState": (_ffi.RgcnState, [f[0] for f in _ffi.RgcnState._fields_])}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "dglmi.h"', "int main(void) {"]
    for cname, (_, names) in fields.items():
        lines.append('printf("%%s %%zu\\n", "%s", sizeof(%s));' % (cname, cname))
        for f in names:
            lines.append('printf("%%s.%%s %%zu\\n", "%s", "%s", offsetof(%s, %s));' % (cname, f, cname, f))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = dict(l.rsplit(" ", 1) for l in subprocess.check_output([str(exe)]).decode().split("\n") if l)
    for cname, (cls, names) in fields.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for f in names:
            assert int(got["%s.%s" % (cname, f)]) == getattr(cls, f).offset, (cname, f)


def test_64bit_graph_selection():
    """graph_index.py:941-952 switches to int64 ids at 2^31 nodes or edges.  Device
    node ids stay int32, so 2^31 nodes raise DGLError; 2^31 edges (or asbits(64))
    select the 64-bit layout: int64 offsets and edge ids (checked on the GPU in
    tests/test_int64_gpu.py)."""
    from dgl.graph_index import device_block_gidx
    g = GraphIndex(2 ** 31)
    assert g.bits_needed() == 64
    with pytest.raises(dgl.DGLError, match="2\\^31 or more nodes"):
        g.get_immutable_gidx("cuda:0")
    tiny = th.zeros(1, dtype=th.int32)
    with pytest.raises(dgl.DGLError, match="2\\^31 or more nodes"):
        device_block_gidx(2 ** 31, 4, tiny, tiny)
    assert GraphIndex(2 ** 31 - 2).bits_needed() == 32
    small = GraphIndex(3)
    small.add_edges([0, 1], [1, 2])
    assert small.device_bits() == 32
    wide = small.asbits(64)
    assert wide.device_bits() == 64 and small.device_bits() == 32
    assert wide.number_of_edges() == 2 and wide.asbits(32).device_bits() == 32
    with pytest.raises(dgl.DGLError, match="Invalid bit width"):
        small.asbits(16)
    from dgl.graph import _PartialIndex
    assert _PartialIndex(4, [0], [1], [2 ** 31]).bits_needed() == 64
    assert _PartialIndex(4, [0], [1], [5]).bits_needed() == 32


def test_rgcn_fused_ok_matches_the_kernel_rule():
    """dgl.kernel.rgcn_fused_ok restates hack_kernels.hip rgcn_fused_ok (20480 LDS floats
    of weights): C5's 4 relations + self-loop at 64 -> 64 fit, a sixth matrix does not."""
    from dgl import kernel as K
    assert K.rgcn_fused_ok(64, 64, 5) and not K.rgcn_fused_ok(64, 64, 6)
    assert K.rgcn_fused_ok(64, 128, 2) and not K.rgcn_fused_ok(64, 128, 3)
    assert K.rgcn_fused_ok(64, 32, 10) and not K.rgcn_fused_ok(64, 32, 11)
    assert not K.rgcn_fused_ok(32, 64, 1) and not K.rgcn_fused_ok(64, 129, 1)


# kernels_project.hip kTileCfgs: (KB, CB, NS) of the k_project_tile / k_project_glds instances
PROJECT_TILES = [(1, 4, 4), (2, 4, 4), (4, 4, 4), (4, 10, 4), (4, 4, 2), (8, 4, 2), (16, 1, 4),
                 (8, 4, 1), (40, 1, 4), (4, 4, 1), (10, 4, 1), (4, 5, 4)]


def _project_pick(k, n):
    """kernels_project.hip pick_tile restated: the instance of least padded MFMA work,
    an extra column slice priced at 10 %, a k split at 5 %, an unsplit K > 256 at 50 %."""
    best, best_cost = -1, 0.0
    for i, (kb, cb, ns) in enumerate(PROJECT_TILES):
        kp, nsl = (4 // ns) * 16 * kb, ns * 16 * cb
        if k > kp:
            continue
        slices = (n + nsl - 1) // nsl
        cost = (float(kp) * slices * nsl * (1.0 + 0.1 * (slices - 1)) * (1.05 if ns < 4 else 1.0)
                * (1.5 if ns == 4 and 16 * kb > 256 else 1.0))
        if best < 0 or cost < best_cost:
            best, best_cost = i, cost
    return best


def test_project_instance_export(monkeypatch):
    """DGLMIProjectInstance reports the kernel DGLMIProject launches: pick_tile's choice
    (restated above) for every K <= 640, -2 where k_project takes the shape itself, -1
    where there is none; DGLMI_PROJECT_CFG / DGLMI_PROJECT_TILE are read on every call."""
    L = _ffi.lib()
    for name in ("DGLMI_PROJECT_CFG", "DGLMI_PROJECT_GLDS", "DGLMI_PROJECT_TILE"):
        monkeypatch.delenv(name, raising=False)
    widths = [1, 33, 64, 65, 128, 256, 320, 321, 602, 640, 1000]
    picked = set()
    for k in range(1, 641):
        for n in widths:
            direct = k in (16, 32, 64, 128) and n in (64, 128)
            want = -2 if direct else _project_pick(k, n)
            assert L.DGLMIProjectInstance(k, n) == want, (k, n)
            picked.add(want)
    # the cost function never picks these two for K <= 640 at these widths (A/B only)
    assert picked == {-2} | (set(range(12)) - {8, 9})
    for k, n in [(641, 64), (0, 64), (64, 0), (64, (1 << 20) + 1)]:
        assert L.DGLMIProjectInstance(k, n) == -1 and not L.DGLMIProjectSupported(k, n)
    assert L.DGLMIProjectInstance(640, 1 << 20) >= 0
    # the tile kernel for the shapes k_project covers
    monkeypatch.setenv("DGLMI_PROJECT_TILE", "1")
    for k in (16, 32, 64, 128):
        for n in (64, 128):
            assert L.DGLMIProjectInstance(k, n) == _project_pick(k, n) >= 0
    monkeypatch.delenv("DGLMI_PROJECT_TILE")
    # a forced instance where K fits it (any N: more column slices), the pick elsewhere
    for i, (kb, cb, ns) in enumerate(PROJECT_TILES):
        kp = (4 // ns) * 16 * kb
        monkeypatch.setenv("DGLMI_PROJECT_CFG", str(i))
        for n in (1, 65, 1000):
            assert L.DGLMIProjectInstance(kp, n) == i
            assert L.DGLMIProjectInstance(kp - 1, n) == i
            assert L.DGLMIProjectInstance(kp + 1, n) == (_project_pick(kp + 1, n) if kp < 640 else -1)
        assert L.DGLMIProjectInstance(64, 64) == -2
    monkeypatch.setenv("DGLMI_PROJECT_CFG", "12")
    assert L.DGLMIProjectInstance(602, 64) == _project_pick(602, 64) == 10


def test_gatconv_fused_route_limits():
    """GATConv takes the fused kernels only where they apply: 32-bit device CSRs, and
    with attention dropout in training gathered tables below 2^31 elements (the
    dropout walks have 32-bit offsets only, capi.cpp gat_set_dropout), a plain
    nn.Dropout below p = 1 and, for the module's own mask, edge ids that index it."""
    from types import SimpleNamespace
    import torch
    from dgl.nn.pytorch import GATConv, FusedGATConv
    g32 = SimpleNamespace(in_csr=SimpleNamespace(bits=32), eid_perm=True)
    g64 = SimpleNamespace(in_csr=SimpleNamespace(bits=64), eid_perm=True)
    gview = SimpleNamespace(in_csr=SimpleNamespace(bits=32), eid_perm=False)
    big = (1 << 31) // 64
    for mask in ("module", "hashed"):
        conv = GATConv(16, 8, 8, attn_drop=0.5)
        conv.attn_drop_mask = mask
        conv.train()
        assert conv._fused_route(g32, big - 1) and not conv._fused_route(g32, big)
        assert not conv._fused_route(g64, 10)
        # the module's keep words are indexed by edge id: a view whose CSR data are not
        # its own edge ids takes the composition; the hashed mask does not care
        assert conv._fused_route(gview, 10) == (mask == "hashed")
        conv.eval()
        assert conv._fused_route(g32, big)
        conv.use_fused = False
        assert not conv._fused_route(g32, 10)
    # p = 1 (every weight dropped) and a dropout module of another type: the composition
    conv = GATConv(16, 8, 8, attn_drop=1.0).train()
    assert not conv._fused_route(g32, 10)
    conv = GATConv(16, 8, 8, attn_drop=0.5).train()
    conv.attn_drop = torch.nn.AlphaDropout(0.5)
    assert not conv._fused_route(g32, 10)
    # FusedGATConv never applies attn_drop (fusedGatConv.py:80,152): no dropout limits
    conv = FusedGATConv(16, 8, 8, attn_drop=0.5).train()
    assert conv._fused_route(g32, big) and conv._fused_route(gview, 10)
    assert not conv._fused_route(g64, 10)


def _fused_gat_entry_calls(g, arrays, keep_bits=32, draw=None):
    """name -> call of each of the twelve fused GAT entries on graph ``g``: ``arrays`` maps
    an argument's role to its DGLMIArray ("grad" for every backward-only array); one keep
    word per edge of ``keep_bits`` bits, ``draw`` a DGLMIDropoutDraw or None (null)."""
    L = _ffi.lib()
    G = ctypes.byref(g)
    A = {k: ctypes.byref(v) for k, v in arrays.items()}
    head = [G, A["ft"], A["el"], A["er"], 0.2]
    state = [A["out"], A["mx"], A["sm"]]
    slopes = [A["lf"], A["ls"]]
    grads = [A["grad"]] * 4
    keep = (ctypes.c_uint32 * 1)()
    D = ctypes.byref(draw) if draw is not None else None
    mid = {"": [], "Dropout": [0.5, 7], "Keep": [keep, keep_bits, 0, 2.0], "Draw": [D]}
    calls = {}
    for infix, m in mid.items():
        s = slopes if infix else []
        calls["DGLMIFusedGat%sForward" % infix] = head + m + state + s + [None]
        calls["DGLMIFusedGat%sBackward" % infix] = head + m + state + s + grads + [None]
    calls["DGLMIFusedGatForwardEx"] = head + state + slopes + [None]
    calls["DGLMIFusedGatBackwardEx"] = head + state + slopes + grads + [None]
    calls["DGLMIFusedGatKernel"] = [G, A["ft"], A["el"], A["er"], A["sm"], A["mx"], A["out"], 0.2, None]
    calls["DGLMIKernelBackwardFusedGat"] = ([G, A["ft"], A["el"], A["er"], A["sm"], A["mx"], A["out"]]
                                            + grads + [0.2, None])
    assert len(calls) == 12
    return {name: (lambda f=getattr(L, name), a=args: f(*a)) for name, args in calls.items()}


def _array(*shape):
    """A DGLMIArray of ``shape`` with no data (zero rows)."""
    a = _ffi.Array()
    a.ndim = len(shape)
    for i, s in enumerate(shape):
        a.shape[i] = s
    return a


def test_fused_gat_entries_refuse_without_device():
    """Every fused GAT entry refuses a 64-bit graph, the Keep entries a keep word width of
    0 and the Draw entries a null draw -- all before any device work."""
    g = _ffi.Graph()
    g.num_bits = 64
    blank = {k: _ffi.Array() for k in ("ft", "el", "er", "out", "mx", "sm", "lf", "ls", "grad")}
    for name, call in _fused_gat_entry_calls(g, blank, draw=_ffi.DropoutDraw()).items():
        assert call() == -1, name
        assert "fused GAT needs a graph of fewer than 2^31 edges" in _ffi.last_error(), name
    # a well-formed call on a 32-bit graph without rows: only the dropout value is wrong
    H, D = 8, 8
    indptr = (ctypes.c_int32 * 1)()
    g = _ffi.Graph()
    g.num_bits = 32
    g.in_csr.indptr = g.out_csr.indptr = ctypes.addressof(indptr)
    empty = {"ft": _array(0, H, D), "el": _array(0, H, 1), "er": _array(0, H, 1), "out": _array(0, H, D),
             "mx": _array(0, H), "sm": _array(0, H), "lf": _array(0, H, D), "ls": _array(0, H),
             "grad": _array(0, H, D)}
    calls = _fused_gat_entry_calls(g, empty, keep_bits=0)
    for name in ("DGLMIFusedGatKeepForward", "DGLMIFusedGatKeepBackward"):
        assert calls[name]() == -1, name
        assert "keep_bits must be 8, 16 or 32" in _ffi.last_error(), name
    for name in ("DGLMIFusedGatDrawForward", "DGLMIFusedGatDrawBackward"):
        assert calls[name]() == -1, name
        assert name + ": draw is required" in _ffi.last_error(), name


def test_fused_gat_dropout_value():
    """dgl.kernel.GatDropout: each maker names its entries and says whether its backward
    needs the forward's slope aggregates; dgl.backend.fused_gat refuses keep words
    without their scale before any device call."""
    from types import SimpleNamespace
    import dgl.backend as B
    from dgl import kernel as K
    hashed = K.GatDropout.hashed(0.5, -1)
    keep = K.GatDropout.keep(th.zeros(3, dtype=th.uint8), 2.0, True)
    draw = K.GatDropout.draw(_ffi.DropoutDraw())
    assert [(d.infix, d.needs_slopes) for d in (hashed, keep, draw)] == \
        [("Dropout", True), ("Keep", True), ("Draw", False)]
    p, seed = hashed.c_args(3)
    assert p == 0.5 and seed.value == 2 ** 64 - 1  # the seed's low 64 bits
    assert len(draw.c_args(3)) == 1
    with pytest.raises(dgl.DGLError, match="uint8 / int16 / int32 ROCm tensor"):
        keep.c_args(3)  # keep words live on the device
    gidx = SimpleNamespace(in_csr=SimpleNamespace(bits=32, nnz=3))
    ft, el = th.zeros(2, 4, 8), th.zeros(2, 4, 1)
    with pytest.raises(dgl.DGLError, match="keep needs keep_scale"):
        B.fused_gat(gidx, ft, el, el, 0.2, keep=th.zeros(3, dtype=th.uint8))


def test_workspace_bytes_match_recorded_layout():
    """DGLMIKernelWorkspaceBytes / DGLMIEdgeSoftmaxWorkspaceBytes over edge counts around
    the chunk sizes and past 2^31, every row-slot width and every softmax head count:
    callers may pass their own workspace, so the sizes (carries rounded up to 16 B, one
    counter per chunk; csrc/internal.h CarryLayout) stay what they were when
    tests/golden/workspace_bytes.json was recorded (from the build before CarryLayout)."""
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "workspace_bytes.json")))
    L = _ffi.lib()

    def csr(rows, nnz):
        return ctypes.byref(_ffi.CSR(rows, rows, nnz, None, None, None, None))

    nnzs = {1, 7, 8, 9, 4095, 4096, 4097, 10 ** 6, 10 ** 8, 3 * 10 ** 9}
    assert {e[0] for e in want["kernel"]} == nnzs and {e[1] for e in want["kernel"]} == {1, 6, 15, 16, 64, 602}
    assert {e[0] for e in want["softmax"]} == nnzs and {e[2] for e in want["softmax"]} == {1, 2, 4, 8, 16}
    assert len(want["kernel"]) == 60 and len(want["softmax"]) == 100
    for nnz, f, nbytes in want["kernel"]:
        assert L.DGLMIKernelWorkspaceBytes(csr(1000, nnz), f) == nbytes, (nnz, f)
    for nnz, rows, h, nbytes in want["softmax"]:
        assert L.DGLMIEdgeSoftmaxWorkspaceBytes(csr(rows, nnz), h) == nbytes, (nnz, rows, h)
