#!/usr/bin/env python3
"""Bit-for-bit A/B of the chunked walks' fixups between two library builds.

--save DIR runs, on the build DGL_LIBRARY_PATH selects (default: the in-tree one), every
case of tests/test_fixup_segments_gpu.py on its three graph variants and the star graphs
of tests/test_hub_rows_gpu.py (3 M-edge copy_u sum with its source gradient, 2 M-edge max,
fused GAT stars in both directions, 1 M-edge edge softmax), all from inputs drawn on the
CPU, and writes every output and gradient to DIR/<case>.npz.  --compare A B requires
np.array_equal on every array of two such directories and prints the list and the verdict
as one JSON line (exit status 1 on any difference)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), ROOT, os.path.join(ROOT, "dgl-hack_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402


def stars():
    import torch as th
    import dgl
    import dgl.backend as B
    import dgl.function as fn
    from dgl.nn.pytorch import edge_softmax
    from test_hub_rows_gpu import DEV, star

    def rand(seed, *shape):
        return th.from_numpy(np.random.RandomState(seed).uniform(-1, 1, shape).astype(np.float32)).to(DEV)

    def graph(n, m, hub, reverse=False):
        src, dst = star(n, m, hub, reverse=reverse)
        g = dgl.DGLGraph()
        g.add_nodes(n)
        g.add_edges(src, dst)
        return g, len(src)

    g, _ = graph(100_000, 3_000_000, 777)
    x = rand(1, 100_000, 64).requires_grad_()
    g.ndata["x"] = x
    g.update_all(fn.copy_u("x", "m"), fn.sum("m", "h"))
    (gx,) = th.autograd.grad(g.ndata["h"], x, rand(2, 100_000, 64))
    yield "star_sum", {"out": g.ndata["h"].detach(), "grad_src": gx}

    g, _ = graph(100_000, 2_000_000, 31)
    g.ndata["x"] = rand(3, 100_000, 64)
    g.update_all(fn.copy_u("x", "m"), fn.max("m", "h"))
    yield "star_max", {"out": g.ndata["h"]}

    for reverse in (False, True):
        g, _ = graph(50_000, 200_000, 123, reverse)
        leaves = [rand(4, 50_000, 4, 4).requires_grad_(), rand(5, 50_000, 4, 1).requires_grad_(),
                  rand(6, 50_000, 4, 1).requires_grad_()]
        out = B.fused_gat(g, *leaves, 0.2)
        gf = th.autograd.grad(out, leaves, rand(7, 50_000, 4, 4))
        yield "star_gat_reverse%d" % reverse, {"out": out.detach(), "g_ft": gf[0], "g_el": gf[1], "g_er": gf[2]}

    g, m = graph(50_000, 1_000_000, 7)
    e = (4 * rand(8, m, 4, 1)).requires_grad_()
    a = edge_softmax(g, e)
    (ge,) = th.autograd.grad(a, e, rand(9, m, 4, 1))
    yield "star_softmax", {"out": a.detach(), "grad": ge}


def save(out_dir):
    import torch as th
    import test_fixup_segments_gpu as T
    os.makedirs(out_dir, exist_ok=True)
    names = []

    def put(name, outs):
        th.cuda.synchronize()
        np.savez(os.path.join(out_dir, name + ".npz"), **{k: v.detach().cpu().numpy() for k, v in outs.items()})
        names.extend("%s/%s" % (name, k) for k in outs)

    for case in T.CASES:
        for variant in T.VARIANTS:
            put("%s_%s" % (case, variant), T.run_case(case, variant))
    for name, outs in stars():
        put(name, outs)
    print(json.dumps({"lib": os.environ.get("DGL_LIBRARY_PATH", "in-tree"), "arrays": len(names)}), flush=True)


def compare(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    arrays, differ = [], []
    if fa != fb:
        differ.append("file lists differ")
    for f in fa:
        if f not in fb:
            continue
        A, B = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        if sorted(A.files) != sorted(B.files):
            differ.append(f)
        for k in A.files:
            name = "%s/%s" % (f[:-4], k)
            arrays.append(name)
            # np.array_equal and the same bytes: a -0.0 or another NaN is a difference too
            if k not in B.files or not np.array_equal(A[k], B[k], equal_nan=True) or A[k].tobytes() != B[k].tobytes():
                differ.append(name)
    print(json.dumps({"arrays": arrays, "differ": differ, "bit_equal": not differ}), flush=True)
    return 1 if differ else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--save", default=None, metavar="DIR")
    ap.add_argument("--compare", nargs=2, default=None, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    save(args.save)
