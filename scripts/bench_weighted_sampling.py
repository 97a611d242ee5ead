#!/usr/bin/env python3
"""Times weighted neighbour sampling (both modes) and select_topk against the torch-op
formulation a user would write on the same device without them, and against the uniform
``sample_neighbors`` on the same graph and seeds:

  with replacement:    the seeds' in-edges expanded, a per-seed running sum of the weights
                       (one global ``cumsum`` minus the row's start), ``fanout`` uniform
                       targets per seed, ``searchsorted``, two gathers;
  without replacement: the expansion, one exponential key ``-log(u) / w`` per edge (zero
                       weights get +inf), a sort by (seed, key), the first ``fanout`` of
                       every seed kept;
  top-k:               the expansion, a sort by (seed, -weight), the first ``k`` kept.

Shapes: those of scripts/bench_sampling.py -- an RMAT graph of 2^20 nodes and 16 M edges
(a, b, c = 0.57, 0.19, 0.19); 1,024 and 8,192 seeds; fan-outs 10 and 25.  Weights: float32,
uniform in (0, 1) with a tenth of the edges at 0.  Each line times the whole call on every
side, the size readback included.

Method: device events around windows of about 40 ms of calls, the sides' windows
alternating, the median of 5 windows with the fastest and slowest beside it.  The ratios are
recorded, not gated.  Writes profiles/weighted_sampling_bench.json.

  python scripts/bench_weighted_sampling.py [--out profiles/weighted_sampling_bench.json]
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
from bench_knn import compare  # noqa: E402
from bench_sampling import rmat_edges  # noqa: E402


def _expand(indptr, seeds):
    """(slot, CSR position, offset of the slot's first entry) of every in-edge of the seeds."""
    start = indptr[seeds]
    deg = indptr[seeds + 1] - start
    off = th.cumsum(deg, 0) - deg
    slot = th.arange(seeds.shape[0], device=seeds.device).repeat_interleave(deg)
    rank = th.arange(slot.shape[0], device=seeds.device) - off[slot]
    return slot, rank + start[slot], rank, off, deg


def torch_weighted_replace(indptr, indices, data, weight, seeds, fanout):
    slot, pos, _, off, deg = _expand(indptr, seeds)
    w = weight[data[pos].long()].double()
    run = th.cumsum(w, 0)
    before = th.cat([run.new_zeros(1), run])[off]  # the running sum ahead of every slot
    end = th.cat([run.new_zeros(1), run])[off + deg]
    live = end > before
    target = before[:, None] + th.rand(seeds.shape[0], fanout, device=seeds.device,
                                       dtype=th.float64) * (end - before)[:, None]
    hit = th.searchsorted(run, target[live].reshape(-1), right=True).clamp_(max=max(run.shape[0] - 1, 0))
    p = pos[hit]
    return indices[p], seeds[live].repeat_interleave(fanout), data[p]


def _first_of_every_slot(key, slot, rank_limit, off):
    order = th.argsort(key)
    n = order.shape[0]
    keep = order[(th.arange(n, device=key.device) - off[slot]) < rank_limit]
    return keep


def torch_weighted_no_replace(indptr, indices, data, weight, seeds, fanout):
    slot, pos, _, off, _ = _expand(indptr, seeds)
    w = weight[data[pos].long()].double()
    e = -th.log(th.rand(w.shape[0], device=w.device, dtype=th.float64)) / w  # w = 0: +inf
    # keys inside [slot, slot + 1): a monotone map of e, +inf at the top
    key = slot.double() + e / (1.0 + e)
    key = th.where(th.isfinite(e), key, slot.double() + 1.0 - 2.0 ** -40)
    keep = _first_of_every_slot(key, slot, fanout, off)
    keep = keep[w[keep] > 0]
    p = pos[keep]
    return indices[p], seeds[slot[keep]], data[p]


def torch_topk(indptr, indices, data, weight, seeds, k):
    slot, pos, _, off, _ = _expand(indptr, seeds)
    w = weight[data[pos].long()].double()
    order = th.argsort(-w, stable=True)  # by weight, then by (slot, position)
    order = order[th.argsort(slot[order], stable=True)]
    n = order.shape[0]
    keep = order[(th.arange(n, device=w.device) - off[slot]) < k]
    p = pos[keep]
    return indices[p], seeds[slot[keep]], data[p]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_sampling_bench.json"))
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=16 * 2 ** 20)
    args = ap.parse_args()
    if not th.cuda.is_available():
        raise SystemExit("bench_weighted_sampling needs the GPU: nothing is timed without one")
    dev = th.device("cuda:0")
    th.manual_seed(0)
    n = 2 ** args.scale
    src, dst = rmat_edges(args.scale, args.edges, dev)
    g = dgl.DGLGraph.from_device_coo(src, dst, n)
    csr = g._graph.get_immutable_gidx(dev).in_csr
    indptr, indices, data = csr.indptr.long(), csr.indices, csr.data
    weight = th.rand(args.edges, device=dev)
    weight[th.rand(args.edges, device=dev) < 0.1] = 0
    res = {"device": th.cuda.get_device_name(0),
           "graph": {"nodes": n, "edges": args.edges, "max_in_degree": int(csr.degrees().max())},
           "weights": "float32, uniform in (0, 1), a tenth of the edges at 0",
           "timing": "device events around windows of about %g ms of calls, median (and min, "
                     "max) of %d alternating windows" % (args.window_ms, args.rounds),
           "lines": {}}

    def line(name, ours, torch_fn, uniform):
        a, b, c = compare([ours, torch_fn, uniform], args.window_ms, args.rounds)
        rec = {"ours": a, "torch": b, "uniform_sample_neighbors": c,
               "torch_over_ours": b["ms"] / a["ms"], "ours_over_uniform": a["ms"] / c["ms"],
               "edges": int(ours()[1].shape[0])}
        res["lines"][name] = rec
        print(name, json.dumps(rec), flush=True)

    for S in (1024, 8192):
        seeds = th.randperm(n, device=dev)[:S]
        seeds32 = seeds.int()
        for fanout in (10, 25):
            for replace in (True, False):
                tfn = torch_weighted_replace if replace else torch_weighted_no_replace
                line("sample_seeds%d_fanout%d_%s" % (S, fanout, "replace" if replace else "no_replace"),
                     lambda: K.sample_neighbors_weighted(csr, seeds32, fanout, replace, weight, 1),
                     lambda: tfn(indptr, indices, data, weight, seeds, fanout),
                     lambda: K.sample_neighbors(csr, seeds32, fanout, replace, 1))
            line("topk_seeds%d_k%d" % (S, fanout),
                 lambda: K.select_topk(csr, seeds32, fanout, weight),
                 lambda: torch_topk(indptr, indices, data, weight, seeds, fanout),
                 lambda: K.sample_neighbors(csr, seeds32, fanout, False, 1))

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"wrote": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
