"""DGLGraph.subgraph against the plain torch formulation on the same device.

Two shapes: a Cluster-GCN step (the union of q of k planted clusters) and half of the nodes of
a power-law graph.  The torch formulation does what a user without the kernel would write on
the device: scatter a position table, gather the selected rows' entries (repeat_interleave
over the degrees), mask by the table, ``nonzero``, index.  Both start from the device out-CSR
and end with (src, dst, parent_eid); the outputs are compared exactly before anything is
timed.  Times are host clocks around work that ends in a synchronise, the two versions
alternating inside one process; a timed window holds as many calls as fill ``--window``
seconds (sized per shape and version from a trial batch); min / median / max over the rounds
are recorded.

    python scripts/bench_subgraph.py --out profiles/subgraph_bench.json
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
from dgl import kernel as K  # noqa: E402
from dgl.data.synthetic import chung_lu_edges, planted_cluster_edges  # noqa: E402


def torch_slice(csr, nodes):
    """The same slice with torch ops: two readbacks (repeat_interleave, nonzero)."""
    n = csr.num_rows
    nodes = nodes.long()
    table = th.full((n,), -1, dtype=th.int64, device=nodes.device)
    table[nodes] = th.arange(nodes.shape[0], device=nodes.device)
    start = csr.indptr[nodes].long()
    deg = csr.indptr[nodes + 1].long() - start
    goff = th.cumsum(deg, 0) - deg
    slot = th.repeat_interleave(th.arange(nodes.shape[0], device=nodes.device), deg)
    entry = th.arange(slot.shape[0], device=nodes.device) - goff[slot] + start[slot]
    pos = table[csr.indices[entry].long()]
    kept = th.nonzero(pos >= 0).reshape(-1)
    return slot[kept].int(), pos[kept].int(), csr.data[entry[kept]].long()


def measure(name, g, nodes, rounds, window):
    dev = nodes.device
    csr = g._graph.get_immutable_gidx(dev).out_csr
    ours = lambda: K.csr_slice(csr, nodes)[:3]
    theirs = lambda: torch_slice(csr, nodes)
    a, b = ours(), theirs()
    assert all(th.equal(x, y) for x, y in zip(a, b)), "the two formulations disagree"

    def timed(f, calls):
        th.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            f()
        th.cuda.synchronize()
        return (time.perf_counter() - t0) / calls

    times = {"hip": [], "torch": []}
    calls = {}
    for key, f in (("hip", ours), ("torch", theirs)):
        timed(f, 3)
        calls[key] = max(20, int(window / timed(f, 20)) + 1)
    for _ in range(rounds):
        for key, f in (("hip", ours), ("torch", theirs)):
            times[key].append(timed(f, calls[key]) * 1e3)
    rec = {"shape": name, "nodes": g.number_of_nodes(), "edges": g.number_of_edges(),
           "selected": int(nodes.shape[0]), "subgraph_edges": int(a[0].shape[0]),
           "rounds": rounds, "window_s": window, "calls_per_window": calls}
    for key, v in times.items():
        v = sorted(v)
        rec[key + "_ms"] = {"min": v[0], "median": v[len(v) // 2], "max": v[-1]}
    print(json.dumps(rec))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the shapes (rehearsal)")
    args = ap.parse_args()
    dev = th.device("cuda:0")
    recs = []

    n, k, q = int(1_000_000 * args.scale), 1000, 20
    src, dst, part = planted_cluster_edges(n, k, 16 * n, 0.8, 0, dev)
    g = dgl.DGLGraph.from_device_coo(src, dst, n)
    member = th.zeros(k, dtype=th.bool, device=dev)
    member[th.randperm(k, generator=th.Generator().manual_seed(1))[:q].to(dev)] = True
    nodes = th.nonzero(member[part]).reshape(-1).int()
    recs.append(measure("cluster_gcn: 20 of 1000 clusters", g, nodes, args.rounds, args.window))
    del g, src, dst

    n = int((1 << 21) * args.scale)
    src, dst = chung_lu_edges(n, 16 * n, 0.6, 0, dev)
    g = dgl.DGLGraph.from_device_coo(src, dst, n)
    nodes = th.randperm(n, generator=th.Generator().manual_seed(2))[:n // 2].to(dev).int()
    recs.append(measure("power-law graph: a random half of the nodes", g, nodes, args.rounds,
                        args.window))

    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": th.cuda.get_device_name(0), "timing": "host clock around a "
                       "synchronise, versions alternating; ms per call", "records": recs}, f, indent=1)


if __name__ == "__main__":
    main()
