#!/usr/bin/env python3
"""Times AtomicConv's fused form (kernels_atomic.hip) against the same module with ``fused =
False`` (the reference's steps: RadialPooling.forward, the message and reduce UDFs on degree
buckets) on the same device, in the same process, on a batched 12-NN graph (dgl.knn_graph of
64 sets of 1,024 points in the unit cube: 65,536 nodes, 786,432 edges, the distances those
of the edges' end points) with 8 atom types (T = 8), at two radial grids:

  small:  K = 5    (a lane group of 8: G = 8 groups per wave)
  wide:   K = 192  (three tiles of 64 filters)

Each side is timed forward (no_grad) and forward + backward (gradients of the distances and
the three filter parameters): device events around windows of calls, the two sides' windows
alternating, the median of `rounds` windows after a warm-up with the fastest and slowest
window beside it, and torch.cuda.max_memory_allocated of one forward + backward per side.
Modelled bytes of the aggregation: fused E (index 12 + distance 4 + 4 T) + 4 N T K; unfused
the three (K, E, 1) filter intermediates written and read, the (E, K) filter values and the
(E, T K) messages written and read, and N T K written.  Writes profiles/atomic_bench.json.

  python scripts/bench_atomicconv.py [--out profiles/atomic_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "dgl-hack_amd"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch as th  # noqa: E402

import dgl  # noqa: E402
from dgl.nn.pytorch import AtomicConv  # noqa: E402
from bench_readout import compare  # noqa: E402

T = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "atomic_bench.json"))
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not th.cuda.is_available():
        raise SystemExit("bench_atomicconv needs the GPU: nothing is timed without one")
    dev = th.device("cuda:0")
    th.manual_seed(0)
    pts = th.rand(64, 1024, 3, device=dev)
    g = dgl.knn_graph(pts, 12)
    src, dst = (t.to(dev).long() for t in g.edges())
    flat = pts.view(-1, 3)
    dist = ((flat[src] - flat[dst]) ** 2).sum(1, keepdim=True).sqrt() * 20   # a few units
    n, e = g.number_of_nodes(), g.number_of_edges()
    feat = th.randint(1, T + 1, (n, 1), device=dev).float()
    res = {"device": th.cuda.get_device_name(0), "nodes": n, "edges": e, "T": T,
           "timing": "device events around windows of about %g ms of calls, median (and min, "
                     "max) of %d alternating windows" % (args.window_ms, args.rounds),
           "shapes": {}}
    for name, nk in (("small", 5), ("wide", 192)):
        conv = AtomicConv(th.linspace(2.0, 6.0, nk), th.linspace(0.0, 6.0, nk),
                          th.full((nk,), 0.5), th.arange(1, T + 1).float()).to(dev)
        d = dist.clone().requires_grad_()
        go = th.randn(n, T * nk, device=dev)
        assert conv._route(g, (feat == conv.features_to_use).float(), d) is not None

        def run(fused, grad):
            def call():
                conv.fused = fused
                if grad:
                    conv.zero_grad()
                    d.grad = None
                with th.enable_grad() if grad else th.no_grad():
                    out = conv(g, feat, d)
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
        rec = {"K": nk, "fused_fwd": f_fwd, "unfused_fwd": r_fwd, "fused_fwd_bwd": f_all,
               "unfused_fwd_bwd": r_all, "unfused_over_fused_fwd": r_fwd["ms"] / f_fwd["ms"],
               "unfused_over_fused_fwd_bwd": r_all["ms"] / f_all["ms"],
               "fused_peak_bytes": peak[True], "unfused_peak_bytes": peak[False],
               "fused_model_bytes": e * (12 + 4 + 4 * T) + 4 * n * T * nk,
               "unfused_model_bytes": 4 * (2 * 3 * e * nk + 2 * e * nk + 2 * e * T * nk + n * T * nk),
               "max_abs_output_difference": diff}
        res["shapes"][name] = rec
        print(name, json.dumps(rec), flush=True)
        del conv, go
        th.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"wrote": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
