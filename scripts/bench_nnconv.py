#!/usr/bin/env python3
"""Times NNConv's fused form (kernels_nnconv.hip) against the reference's step order called
on the builtins directly (u_mul_e of (N, in, 1) with (E, in, out), sum reducer, .sum(1):
what runs, unchanged, without the new kernels) on the same device, in the same process, at
two shapes:

  mpnn:   a dgl.batch of 140 complete graphs of 20 nodes (2,800 nodes, 53,200 edges),
          64 -> 64, edge_func a two-layer MLP (16 -> 128 -> 4096);
  arxiv:  169,343 nodes and 1,166,243 edges with power-law in-degrees, 16 -> 16,
          edge_func a two-layer MLP (8 -> 32 -> 256).

Each side is timed forward (no_grad, edge_func included) and forward + backward (gradients
of feat, efeat and edge_func's parameters): device events around windows of about 300 ms of
calls (the count chosen per side from a first estimate), the two sides' windows
alternating, the median of `rounds` windows after a warm-up with the fastest and slowest
window beside it, and torch.cuda.max_memory_allocated of one forward + backward per side.
The two kernels alone (K.nnconv_aggregate, K.nnconv_backward with both gradients) are
timed the same way; their modelled bytes (forward E in out 4 + the gathers of x and the
rows of out; backward one read and one write of that + the gathers of g and x and dx)
over the kernel time are given as a rate and as a share of the 8 TB/s HBM peak.  Writes
profiles/nnconv_bench.json.

  python scripts/bench_nnconv.py [--out profiles/nnconv_bench.json]
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
import dgl.function as fn  # noqa: E402
from dgl import kernel as K  # noqa: E402
from dgl.nn.pytorch import NNConv  # noqa: E402
from bench_readout import compare  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, the MI355X's spec


def mpnn_case(dev):
    n = 20
    src, dst = np.nonzero(1 - np.eye(n, dtype=np.int64))
    graphs = []
    for _ in range(140):
        g = dgl.DGLGraph()
        g.add_nodes(n)
        g.add_edges(src, dst)
        graphs.append(g)
    return dgl.batch(graphs), dict(fi=64, fo=64, fe=16, hidden=128)


def arxiv_case(dev):
    n, m = 169343, 1166243
    rng = np.random.default_rng(0)
    w = 1.0 / np.arange(1, n + 1) ** 0.8
    dst = rng.choice(n, m, p=w / w.sum()).astype(np.int32)
    src = rng.integers(0, n, m).astype(np.int32)
    g = dgl.DGLGraph.from_device_coo(th.from_numpy(src).to(dev), th.from_numpy(dst).to(dev), n)
    return g, dict(fi=16, fo=16, fe=8, hidden=32)


def builtin_nnconv(g, x, w3):
    """nnconv.py:105-121 on the builtins: no code of the fused path."""
    g = g.local_var()
    g.srcdata['h'] = x.unsqueeze(-1)
    g.edata['w'] = w3
    g.update_all(fn.u_mul_e('h', 'w', 'm'), fn.sum('m', 'neigh'))
    return g.dstdata['neigh'].sum(dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nnconv_bench.json"))
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not th.cuda.is_available():
        raise SystemExit("bench_nnconv needs the GPU: nothing is timed without one")
    dev = th.device("cuda:0")
    th.manual_seed(0)
    res = {"device": th.cuda.get_device_name(0),
           "timing": "device events around windows of about %g ms of calls, median (and min, "
                     "max) of %d alternating windows" % (args.window_ms, args.rounds),
           "hbm_peak_bytes_per_s": HBM_PEAK, "shapes": {}}
    for name, make in (("mpnn", mpnn_case), ("arxiv", arxiv_case)):
        g, s = make(dev)
        n, e, fi, fo = g.number_of_nodes(), g.number_of_edges(), s["fi"], s["fo"]
        mlp = th.nn.Sequential(th.nn.Linear(s["fe"], s["hidden"]), th.nn.ReLU(),
                               th.nn.Linear(s["hidden"], fi * fo))
        conv = NNConv(fi, fo, mlp, "sum", bias=False).to(dev)
        x = th.randn(n, fi, device=dev, requires_grad=True)
        ef = th.randn(e, s["fe"], device=dev, requires_grad=True)
        go = th.randn(n, fo, device=dev)
        with th.no_grad():
            w = conv.edge_nn(ef)
        gidx = conv._route(g, x, w)
        assert gidx is not None, "the fused route must serve the benchmark's shape"

        def run(fused, grad):
            def call():
                if grad:
                    conv.zero_grad()
                    x.grad = ef.grad = None
                with th.enable_grad() if grad else th.no_grad():
                    out = conv(g, x, ef) if fused else \
                        builtin_nnconv(g, x, conv.edge_nn(ef).view(-1, fi, fo))
                if grad:
                    out.backward(go)
                return out
            return call

        diff = float((run(True, False)() - run(False, False)()).abs().max())
        peak = {}
        for side in (True, False):
            run(side, True)()
            th.cuda.synchronize()
            th.cuda.reset_peak_memory_stats()
            run(side, True)()
            th.cuda.synchronize()
            peak[side] = th.cuda.max_memory_allocated()
        f_fwd, r_fwd = compare(run(True, False), run(False, False), args.window_ms, args.rounds)
        f_all, r_all = compare(run(True, True), run(False, True), args.window_ms, args.rounds)
        out, dx, dw = th.empty(n, fo, device=dev), th.empty(n, fi, device=dev), th.empty_like(w)
        xd = x.detach()
        k_fwd, _ = compare(lambda: K.nnconv_aggregate(gidx, xd, w, out), None,
                           args.window_ms, args.rounds)
        k_bwd, _ = compare(lambda: K.nnconv_backward(gidx, xd, w, go, None, dx=dx, dw=dw), None,
                           args.window_ms, args.rounds)
        fwd_b = 4 * (e * fi * fo + e * fi + n * fo)
        bwd_b = 4 * (2 * e * fi * fo + e * fo + e * fi + n * fi)
        for k, b in ((k_fwd, fwd_b), (k_bwd, bwd_b)):
            k["model_bytes"] = b
            k["bytes_per_s"] = b / (k["ms"] * 1e-3)
            k["share_of_hbm_peak"] = k["bytes_per_s"] / HBM_PEAK
        rec = {"nodes": n, "edges": e, **s, "chunk": K.nnconv_chunk(fi, fo, e),
               "w_bytes": 4 * e * fi * fo, "fused_fwd": f_fwd, "builtin_fwd": r_fwd,
               "fused_fwd_bwd": f_all, "builtin_fwd_bwd": r_all,
               "builtin_over_fused_fwd": r_fwd["ms"] / f_fwd["ms"],
               "builtin_over_fused_fwd_bwd": r_all["ms"] / f_all["ms"],
               "fused_peak_bytes": peak[True], "builtin_peak_bytes": peak[False],
               "kernel_aggregate": k_fwd, "kernel_backward": k_bwd,
               "max_abs_output_difference": diff}
        res["shapes"][name] = rec
        print(name, json.dumps(rec), flush=True)
        del w, dw, conv, x, ef
        th.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"wrote": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
