#!/usr/bin/env python3
"""Times RelGraphConv(regularizer="bdd") on the segment kernels (csrc/kernels_rgcn_bdd.hip;
the module's ``use_fused`` branch, forced where ``rgcn_bdd_route`` declines a shape)
against the route it replaces: the same module with ``use_fused = False``, i.e. the
(N, R, out) einsum table plus the typed gather.

  kg:    a synthetic knowledge graph of the link-prediction example's size -- N = 14 541,
         about 620 k edges counting inverse edges, R = 474 relations (237 and their
         inverses, relation frequencies and degrees power-law), 500 -> 500, 100 bases;
  small: 64 -> 64, 8 bases, R = 8 on an arxiv-size power-law graph (169 343 nodes,
         1 166 243 edges).

Per shape and route: forward, and forward + backward (all parameter gradients and the
input gradient), device events around windows of about `--window-ms` of calls, the two
routes' windows alternating, the median of `--rounds` windows after a warm-up with the
fastest and slowest window beside it; the peak of torch.cuda.max_memory_allocated over
one forward + backward above what was allocated before it; and the largest difference
between the two routes' outputs and gradients at the timed sizes.  The segment kernels'
workspaces come from the library's stream-ordered pool and are not in torch's figure:
they are reported from their sizes (carries, weight-gradient partials).  Writes
profiles/rgcn_bdd_bench.json.

  python scripts/bench_rgcn_bdd.py [--out profiles/rgcn_bdd_bench.json] [--shapes kg,small]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "dgl-hack_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch as th  # noqa: E402

import dgl  # noqa: E402
import dgl.backend as B  # noqa: E402
from dgl import kernel as K  # noqa: E402
from dgl.nn.pytorch import RelGraphConv  # noqa: E402


def powerlaw_ids(rng, n, m, a):
    """m ids in [0, n), the i-th most frequent about (i + 1)^-a of the draws."""
    p = (np.arange(n) + 1.0) ** -a
    return rng.permutation(n)[rng.choice(n, m, p=p / p.sum())]


def knowledge_graph(rng):
    n, m, r = 14541, 310116, 237
    src, dst = powerlaw_ids(rng, n, m, 0.8), powerlaw_ids(rng, n, m, 0.8)
    rel = powerlaw_ids(rng, r, m, 1.0)
    return n, np.concatenate([src, dst]), np.concatenate([dst, src]), np.concatenate([rel, rel + r]), 2 * r


def small_block_graph(rng):
    n, m, r = 169343, 1166243, 8
    return n, rng.integers(0, n, m), powerlaw_ids(rng, n, m, 0.6), rng.integers(0, r, m), r


def window(fn, reps):
    a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def compare(fns, window_ms, rounds):
    sides = []
    for fn in fns:
        fn()
        fn()
        th.cuda.synchronize()
        est = window(fn, 2)
        sides.append({"fn": fn, "reps": int(min(500, max(2, np.ceil(window_ms / est)))), "t": []})
    for _ in range(rounds):
        for side in sides:
            side["t"].append(window(side["fn"], side["reps"]))
    return [{"ms": float(np.median(s["t"])), "min_ms": float(min(s["t"])), "max_ms": float(max(s["t"])),
             "reps": s["reps"]} for s in sides]


def run_shape(name, graph, fi, fo, nb, args, dev):
    rng = np.random.default_rng(0)
    n, src, dst, rel, R = graph(rng)
    g = dgl.DGLGraph()
    g.add_nodes(n)
    g.add_edges(src, dst)
    etypes = th.from_numpy(rel).to(dev)
    th.manual_seed(0)
    conv = RelGraphConv(fi, fo, R, "bdd", nb, self_loop=True).to(dev)
    x = th.randn(n, fi, device=dev)
    deg = np.bincount(dst, minlength=n)
    norm = th.from_numpy(1.0 / deg[dst]).float().reshape(-1, 1).to(dev)
    go = th.randn(n, fo, device=dev)
    rec_routed = B.rgcn_bdd_route(g, x, (R, fi, fo, nb), norm, etypes) is not None

    def segment_forward(xi):
        """RelGraphConv.forward's bdd branch, also where the route function declines."""
        route = B.rgcn_bdd_route(g, xi, (R, fi, fo, nb), norm, etypes, force=True)
        return B.rgcn_bdd_layer(route, xi, conv.weight, conv.h_bias, B.project(xi, conv.loop_weight))

    def step(fused, backward):
        conv.use_fused = False
        xi = x.detach().requires_grad_(backward)
        with th.set_grad_enabled(backward):
            out = segment_forward(xi) if fused else conv(g, xi, etypes, norm)
        if not backward:
            return [out]
        conv.zero_grad(set_to_none=True)
        out.backward(go)
        return [out.detach(), xi.grad] + [p.grad for p in conv.parameters()]

    rec = {"nodes": n, "edges": int(len(src)), "relations": R, "in": fi, "out": fo, "bases": nb,
           "route_function_takes_segment_kernels": rec_routed, "table_bytes_N_R_out": n * R * fo * 4}
    peaks = {}
    for label, fused in (("segment_kernels", True), ("einsum_table", False)):
        step(fused, True)
        th.cuda.synchronize()
        th.cuda.reset_peak_memory_stats()
        before = th.cuda.memory_allocated()
        step(fused, True)
        th.cuda.synchronize()
        peaks[label] = int(th.cuda.max_memory_allocated() - before)
    rec["peak_bytes_forward_backward"] = peaks
    chunks = -(-len(src) // K.RGCN_BDD_CHUNK)
    state = g._graph.__dict__["_rgcn_bdd"][2]
    rec["segment_kernels_pool_workspace_bytes"] = {
        "carries": chunks * (max(fi, fo) * 4 + 4),
        "weight_gradient_partials": int(state.c.num_chunks) * fi * (fo // nb) * 4}
    a, b = step(True, True), step(False, True)
    rec["max_abs_difference"] = [float((p - q).abs().max()) for p, q in zip(a, b)]
    rec["max_abs_einsum_table"] = [float(q.abs().max()) for q in b]
    for label, backward in (("forward", False), ("forward_backward", True)):
        new, old = compare([lambda: step(True, backward), lambda: step(False, backward)],
                           args.window_ms, args.rounds)
        rec[label] = {"segment_kernels": new, "einsum_table": old,
                      "einsum_table_over_segment_kernels": old["ms"] / new["ms"]}
    print(name, json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgcn_bdd_bench.json"))
    ap.add_argument("--shapes", default="kg,small")
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not th.cuda.is_available():
        raise SystemExit("bench_rgcn_bdd needs the GPU: nothing is timed without one")
    dev = th.device("cuda:0")
    res = {"device": th.cuda.get_device_name(0),
           "timing": "device events around windows of about %g ms of calls, median (and min, max) "
                     "of %d alternating windows after two warm-up calls per route"
                     % (args.window_ms, args.rounds)}
    shapes = {"kg": (knowledge_graph, 500, 500, 100), "small": (small_block_graph, 64, 64, 8)}
    for name in args.shapes.split(","):
        res[name] = run_shape(name, *shapes[name], args, dev)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"wrote": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
