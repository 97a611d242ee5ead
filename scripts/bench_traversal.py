"""dgl.traversal against a level-synchronous torch formulation on the same device.

Shapes: a batch of random trees (child -> parent edges, topological frontiers: hundreds of
small levels) and a power-law graph (BFS from node 0: a dozen huge levels).  Both kernel
routes are timed (``variant`` 1: wide only; 2: narrow wherever legal, which is also the
shipped choice 0).  The torch formulation is what a user without the kernels would write:
per level, gather the frontier's entries (repeat_interleave over the degrees), mask, and
``unique``; it yields each frontier as a sorted set, not in the queue's order, so it computes
less than the kernels do.  The frontiers are compared as sets before anything is timed.

A sweep over layered graphs (64 levels of w nodes with one out-edge each, so S = G = w at
every level) times variant 1 against 2 for the choice of DGLMITraverseNarrowLimit().

Times are host clocks around calls that end in a readback, the versions alternating inside
one process; min / median / max of ``--rounds`` windows are recorded.

    python scripts/bench_traversal.py --out profiles/traversal_bench.json
"""
import argparse
import json
import os
import sys
import time

import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "dgl-hack_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import dgl  # noqa: E402
from dgl.data.synthetic import chung_lu_edges  # noqa: E402


def _rows(csr, frontier):
    start = csr.indptr[frontier].long()
    deg = csr.indptr[frontier + 1].long() - start
    slot = th.repeat_interleave(th.arange(frontier.shape[0], device=frontier.device), deg)
    goff = th.cumsum(deg, 0) - deg
    entry = th.arange(slot.shape[0], device=frontier.device) - goff[slot] + start[slot]
    return csr.indices[entry].long()


def torch_bfs(g, source):
    csr = g._graph.get_immutable_gidx(source.device).out_csr
    visited = th.zeros(csr.num_rows, dtype=th.bool, device=source.device)
    frontier, out = source.long(), []
    visited[frontier] = True
    while frontier.shape[0]:
        out.append(frontier)
        col = _rows(csr, frontier)
        frontier = th.unique(col[~visited[col]])
        visited[frontier] = True
    return out


def torch_topo(g, dev):
    gidx = g._graph.get_immutable_gidx(dev)
    csr = gidx.out_csr
    rem = (gidx.in_csr.indptr[1:] - gidx.in_csr.indptr[:-1]).long()
    frontier, out = th.nonzero(rem == 0).reshape(-1), []
    while frontier.shape[0]:
        out.append(frontier)
        col = _rows(csr, frontier)
        rem.index_add_(0, col, th.full_like(col, -1))
        touched = th.unique(col)
        frontier = touched[rem[touched] == 0]
    return out


def timed(f, calls):
    th.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        f()
    th.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def measure(name, g, versions, rounds, window):
    ref = [f.sort().values for f in versions["variant2"]()]
    for key, f in versions.items():
        got = f()
        assert len(got) == len(ref) and all(th.equal(a.sort().values, b) for a, b in zip(got, ref)), key
    calls, times = {}, {k: [] for k in versions}
    for key, f in versions.items():
        calls[key] = max(3, int(window / timed(f, 2)) + 1)
    for _ in range(rounds):
        for key, f in versions.items():
            times[key].append(timed(f, calls[key]) * 1e3)
    rec = {"shape": name, "nodes": g.number_of_nodes(), "edges": g.number_of_edges(),
           "levels": len(ref), "largest_frontier": max(int(f.shape[0]) for f in ref),
           "rounds": rounds, "window_s": window, "calls_per_window": calls}
    for key, v in times.items():
        v = sorted(v)
        rec[key + "_ms"] = {"min": v[0], "median": v[len(v) // 2], "max": v[-1]}
    print(json.dumps(rec))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the shapes (rehearsal)")
    args = ap.parse_args()
    dev = th.device("cuda:0")
    gen = th.Generator().manual_seed(0)
    recs = []

    # 256 random trees of 1000 nodes: the parent of node c is one of the three nodes before it
    trees, size = max(1, int(256 * args.scale)), 1000
    c = th.arange(1, size)
    parent = c - 1 - (th.rand(trees, size - 1, generator=gen) * th.minimum(c, th.tensor(3))).long()
    base = (th.arange(trees) * size).reshape(-1, 1)
    src, dst = (c + base).reshape(-1).int().to(dev), (parent + base).reshape(-1).int().to(dev)
    g = dgl.DGLGraph.from_device_coo(src, dst, trees * size)
    topo = {"variant%d" % v: (lambda v=v: dgl.topological_nodes_generator(g, variant=v)) for v in (1, 2)}
    topo["torch"] = lambda: torch_topo(g, dev)
    recs.append(measure("batched trees: topological frontiers", g, topo, args.rounds, args.window))

    n = int((1 << 20) * args.scale)
    src, dst = chung_lu_edges(n, 16 * n, 0.6, 0, dev)
    g = dgl.DGLGraph.from_device_coo(src, dst, n)
    seed = th.zeros(1, dtype=th.int64, device=dev)
    bfs = {"variant%d" % v: (lambda v=v: dgl.bfs_nodes_generator(g, seed, variant=v)) for v in (1, 2)}
    bfs["torch"] = lambda: torch_bfs(g, seed)
    recs.append(measure("power-law graph: BFS from node 0", g, bfs, args.rounds, args.window))

    for w in (64, 256, 1024, 2048, 4096):
        levels = 64
        u = th.arange(w * (levels - 1))
        v = w + (u // w) * w + th.randperm(w, generator=gen)[u % w]
        g = dgl.DGLGraph.from_device_coo(u.int().to(dev), v.int().to(dev), w * levels)
        src0 = th.arange(w, device=dev)
        sweep = {"variant%d" % k: (lambda k=k: dgl.bfs_nodes_generator(g, src0, variant=k)) for k in (1, 2)}
        recs.append(measure("sweep: 64 levels of S = G = %d" % w, g, sweep, args.rounds, args.window))

    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": th.cuda.get_device_name(0), "timing": "host clock around calls that "
                       "end in a readback, versions alternating; ms per traversal",
                       "narrow_limit": dgl.kernel.traverse_narrow_limit(), "records": recs}, f, indent=1)


if __name__ == "__main__":
    main()
