#!/usr/bin/env python3
"""Times GMMConv's fused form (aggregate first on kernels_gmm.hip, one GEMM after) against
``fused = False`` (the reference's step order on the builtins: project to K * out, u_mul_e
+ reducer over (N, K, out), sum over K) on the same device, in the same process, at two
shapes:

  knn:    256 point sets of 1,024 points in the plane, 8 nearest neighbours each
          (262,144 nodes, 2,097,152 edges), pseudo = the neighbour's offset, K = 25,
          dim = 2, 64 -> 64;
  arxiv:  169,343 nodes and 1,166,243 edges with power-law in-degrees, random pseudo,
          K = 3, dim = 2, 128 -> 128.

Each side is timed forward and forward + backward (gradients of feat, pseudo, mu,
inv_sigma, fc.weight and bias): device events around windows of about 40 ms of calls (the
count chosen per side from a first estimate), the two sides' windows alternating, the
median of `rounds` windows after a warm-up, with the fastest and slowest window beside
it.  Beside the times: the modelled gather + write bytes of the aggregation (reference
E K out + N K out floats, fused E in + N K in) and their ratio, and the largest
difference between the two sides' outputs on the timed inputs.  Writes
profiles/gmm_bench.json.

  python scripts/bench_gmm.py [--out profiles/gmm_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "dgl-hack_amd"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch as th  # noqa: E402

import dgl  # noqa: E402
from dgl.nn.pytorch import GMMConv  # noqa: E402
from bench_readout import compare  # noqa: E402


def knn_case(dev):
    pts = th.rand(256, 1024, 2, device=dev)
    g = dgl.knn_graph(pts, 8)
    csr = g._graph.get_immutable_gidx(dev).in_csr
    flat = pts.view(-1, 2)
    pseudo = th.empty(csr.nnz, 2, device=dev)
    pseudo[csr.data.long()] = flat[csr.indices.long()] - flat[csr.rows.long()]
    return g, pseudo * 16, dict(K=25, dim=2, fi=64, fo=64)   # offsets of a few sigma


def arxiv_case(dev):
    n, m = 169343, 1166243
    rng = np.random.default_rng(0)
    w = 1.0 / np.arange(1, n + 1) ** 0.8
    dst = rng.choice(n, m, p=w / w.sum()).astype(np.int32)
    src = rng.integers(0, n, m).astype(np.int32)
    g = dgl.DGLGraph.from_device_coo(th.from_numpy(src).to(dev), th.from_numpy(dst).to(dev), n)
    return g, th.randn(m, 2, device=dev), dict(K=3, dim=2, fi=128, fo=128)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmm_bench.json"))
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not th.cuda.is_available():
        raise SystemExit("bench_gmm needs the GPU: nothing is timed without one")
    dev = th.device("cuda:0")
    th.manual_seed(0)
    res = {"device": th.cuda.get_device_name(0),
           "timing": "device events around windows of about %g ms of calls, median (and min, "
                     "max) of %d alternating windows" % (args.window_ms, args.rounds),
           "shapes": {}}
    for name, make in (("knn", knn_case), ("arxiv", arxiv_case)):
        g, pseudo, s = make(dev)
        n, e = g.number_of_nodes(), g.number_of_edges()
        conv = GMMConv(s["fi"], s["fo"], s["dim"], s["K"], "sum").to(dev)
        x = th.randn(n, s["fi"], device=dev, requires_grad=True)
        pseudo.requires_grad_()
        go = th.randn(n, s["fo"], device=dev)

        def fwd(fused):
            def run():
                conv.fused = fused
                with th.no_grad():
                    return conv(g, x, pseudo)
            return run

        def both(fused):
            def run():
                conv.fused = fused
                conv.zero_grad()
                x.grad = pseudo.grad = None
                conv(g, x, pseudo).backward(go)
            return run

        diff = float((fwd(True)() - fwd(False)()).abs().max())
        f_fwd, r_fwd = compare(fwd(True), fwd(False), args.window_ms, args.rounds)
        f_all, r_all = compare(both(True), both(False), args.window_ms, args.rounds)
        ref_b = 4 * (e * s["K"] * s["fo"] + n * s["K"] * s["fo"])
        fus_b = 4 * (e * s["fi"] + n * s["K"] * s["fi"])
        rec = {"nodes": n, "edges": e, **s, "fused_fwd": f_fwd, "unfused_fwd": r_fwd,
               "fused_fwd_bwd": f_all, "unfused_fwd_bwd": r_all,
               "unfused_over_fused_fwd": r_fwd["ms"] / f_fwd["ms"],
               "unfused_over_fused_fwd_bwd": r_all["ms"] / f_all["ms"],
               "model_bytes_unfused": ref_b, "model_bytes_fused": fus_b,
               "model_bytes_ratio": ref_b / fus_b, "max_abs_output_difference": diff}
        res["shapes"][name] = rec
        print(name, json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"wrote": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
