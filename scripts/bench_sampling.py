#!/usr/bin/env python3
"""Times device neighbour sampling and block relabelling against the torch-op formulation a
user would write on the same device without them:

  with replacement:    ``indptr[seeds] + floor(rand * deg)`` and two gathers;
  without replacement: the seeds' in-edges expanded, one random key per edge, a sort by
                       (seed, key), the first ``fanout`` of every seed kept;
  relabel:             ``torch.unique`` with inverse, the first occurrence of every id by a
                       scatter-min, an argsort of the first occurrences.

Shapes: an RMAT graph of 2^20 nodes and 16 M edges (a, b, c = 0.57, 0.19, 0.19); 1,024 and
8,192 seeds; fan-outs 10 and 25; both replace modes.  Each line times the whole call on
either side, the size readback included.  The two-layer ``sample_blocks`` step (fan-outs 10
then 25, as examples/graphsage_sampling.py) is timed as a whole for both replace modes.

Method: device events around windows of about 40 ms of calls, the two sides' windows
alternating, the median of 5 windows with the fastest and slowest beside it.  Writes
profiles/sampling_bench.json.

  python scripts/bench_sampling.py [--out profiles/sampling_bench.json]
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
from dgl import kernel as K  # noqa: E402
from bench_knn import compare, spread_gate  # noqa: E402


def rmat_edges(scale, m, dev, a=0.57, b=0.19, c=0.19):
    src = th.zeros(m, dtype=th.int64, device=dev)
    dst = th.zeros(m, dtype=th.int64, device=dev)
    for _ in range(scale):
        r = th.rand(m, device=dev)
        src = src * 2 + (r >= a + b).long()
        dst = dst * 2 + (((r >= a) & (r < a + b)) | (r >= a + b + c)).long()
    return src.int(), dst.int()


def torch_sample_replace(indptr, indices, data, seeds, fanout):
    start = indptr[seeds]
    deg = indptr[seeds + 1] - start
    pos = start[:, None] + (th.rand(seeds.shape[0], fanout, device=seeds.device) *
                            deg[:, None]).long()
    pos = pos[deg > 0].reshape(-1)
    own = seeds[deg > 0].repeat_interleave(fanout)
    return indices[pos], own, data[pos]


def torch_sample_no_replace(indptr, indices, data, seeds, fanout):
    start = indptr[seeds]
    deg = indptr[seeds + 1] - start
    off = th.cumsum(deg, 0) - deg
    slot = th.arange(seeds.shape[0], device=seeds.device).repeat_interleave(deg)
    total = slot.shape[0]
    pos = th.arange(total, device=seeds.device) - off[slot] + start[slot]
    key = slot.double() + th.rand(total, device=seeds.device, dtype=th.float64)
    order = th.argsort(key)
    keep = order[(th.arange(total, device=seeds.device) - off[slot]) < fanout]
    pos = pos[keep]
    return indices[pos], seeds[slot[keep]], data[pos]


def torch_relabel(dst_nodes, src):
    seq = th.cat([dst_nodes, src])
    uniq, inv = th.unique(seq, return_inverse=True)
    P = seq.shape[0]
    first = th.full((uniq.shape[0],), P, dtype=th.int64, device=seq.device)
    first.scatter_reduce_(0, inv, th.arange(P, device=seq.device), "amin")
    order = th.argsort(first)
    new_id = th.empty_like(order)
    new_id[order] = th.arange(order.shape[0], device=seq.device)
    return uniq[order], new_id[inv[dst_nodes.shape[0]:]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampling_bench.json"))
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=16 * 2 ** 20)
    args = ap.parse_args()
    if not th.cuda.is_available():
        raise SystemExit("bench_sampling needs the GPU: nothing is timed without one")
    dev = th.device("cuda:0")
    th.manual_seed(0)
    n = 2 ** args.scale
    src, dst = rmat_edges(args.scale, args.edges, dev)
    g = dgl.DGLGraph.from_device_coo(src, dst, n)
    csr = g._graph.get_immutable_gidx(dev).in_csr
    indptr, indices, data = csr.indptr.long(), csr.indices, csr.data
    res = {"device": th.cuda.get_device_name(0),
           "graph": {"nodes": n, "edges": args.edges, "max_in_degree": int(csr.degrees().max())},
           "timing": "device events around windows of about %g ms of calls, median (and min, "
                     "max) of %d alternating windows" % (args.window_ms, args.rounds),
           "kernels": {}, "sample_blocks": {}}

    for S in (1024, 8192):
        seeds = th.randperm(n, device=dev)[:S]
        seeds32 = seeds.int()
        for fanout in (10, 25):
            for replace in (True, False):
                tfn = torch_sample_replace if replace else torch_sample_no_replace
                ours, theirs = compare(
                    [lambda: K.sample_neighbors(csr, seeds32, fanout, replace, 1),
                     lambda: tfn(indptr, indices, data, seeds, fanout)], args.window_ms, args.rounds)
                _, nbr, _ = K.sample_neighbors(csr, seeds32, fanout, replace, 1)
                r_ours, r_theirs = compare(
                    [lambda: K.block_relabel(seeds32, nbr, n), lambda: torch_relabel(seeds, nbr.long())],
                    args.window_ms, args.rounds)
                rec = {"sample_neighbors": ours, "torch_sample": theirs,
                       "torch_over_sample_neighbors": theirs["ms"] / ours["ms"],
                       "sample_below_torch_by_more_than_spread": spread_gate(ours, theirs),
                       "edges": int(nbr.shape[0]), "block_relabel": r_ours, "torch_relabel": r_theirs,
                       "torch_over_block_relabel": r_theirs["ms"] / r_ours["ms"],
                       "relabel_below_torch_by_more_than_spread": spread_gate(r_ours, r_theirs)}
                name = "seeds%d_fanout%d_%s" % (S, fanout, "replace" if replace else "no_replace")
                res["kernels"][name] = rec
                print(name, json.dumps(rec), flush=True)

        for replace in (True, False):
            def ours_step():
                s, blocks = seeds, []
                for fanout in (10, 25):
                    fr = dgl.sampling.sample_neighbors(g, s, fanout, replace=replace, seed=1)
                    b = dgl.to_block(fr, s)
                    s = b.srcdata[dgl.NID]
                    blocks.insert(0, b)
                return blocks

            def torch_step():
                s, blocks = seeds, []
                tfn = torch_sample_replace if replace else torch_sample_no_replace
                for fanout in (10, 25):
                    nbr, own, eid = tfn(indptr, indices, data, s, fanout)
                    src_nodes, new_src = torch_relabel(s, nbr.long())
                    blocks.insert(0, (src_nodes, new_src, own, eid))
                    s = src_nodes
                return blocks

            ours, theirs = compare([ours_step, torch_step], args.window_ms, args.rounds)
            rec = {"sample_blocks": ours, "torch_sample_blocks": theirs,
                   "torch_over_sample_blocks": theirs["ms"] / ours["ms"],
                   "below_torch_by_more_than_spread": spread_gate(ours, theirs),
                   "input_nodes": int(ours_step()[0].number_of_src_nodes())}
            name = "seeds%d_fanouts10_25_%s" % (S, "replace" if replace else "no_replace")
            res["sample_blocks"][name] = rec
            print(name, json.dumps(rec), flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"wrote": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
