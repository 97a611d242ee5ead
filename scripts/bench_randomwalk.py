#!/usr/bin/env python3
"""Times the device random walk and the visit-count kernel against the torch-op formulation
a user would write on the same device without them:

  walk:   per step a degree lookup (``indptr[v + 1] - indptr[v]``), ``floor(rand * deg)``,
          a gather from ``indices`` and the masks for dead ends and restarts;
  counts: ``torch.unique(return_counts=True)`` on ``slot * N + node`` keys, two stable sorts
          to (slot, count descending, id ascending) and the first k of every slot.

Shapes.  PinSAGE: a bipartite user-item graph whose two ends are drawn from Chung-Lu weights
(``dgl.data.synthetic.chung_lu_edges``), both directions as relations; 4,096 seeds x 200
walks x 3 traversals of 2 hops, restart 0.5 after a traversal, top 10.  DeepWalk: 2^20 walks
of length 40 on a symmetrised Chung-Lu graph.

The walk's two store variants (1: every lane stores its own row, 2: staged in LDS and
flushed row by row) are timed against each other in the same alternating windows, and their
traces compared bitwise.  Rates: a step that finds an edge makes two dependent loads, the
row's bounds in ``indptr`` and the drawn entry of ``indices``; a step at a dead end makes one.

Method: device events around windows of about 40 ms of calls, the sides' windows
alternating, the median of 5 windows with the fastest and slowest beside it.  Writes
profiles/randomwalk_bench.json.

  python scripts/bench_randomwalk.py [--out profiles/randomwalk_bench.json]
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

from dgl import kernel as K  # noqa: E402
from dgl.data.synthetic import chung_lu_edges  # noqa: E402
from dgl.graph_index import device_block_gidx  # noqa: E402
from bench_knn import compare, spread_gate  # noqa: E402


def torch_walk(csrs, path, seeds, probs):
    """``csrs``: (indptr int64, indices) per relation; ``probs``: a float per step or None."""
    n = seeds.shape[0]
    cur = seeds.long()
    alive = th.ones(n, dtype=th.bool, device=seeds.device)
    cols = [cur]
    for t, rel in enumerate(path):
        indptr, indices = csrs[rel]
        v = cur.clamp(min=0)
        start = indptr[v]
        deg = indptr[v + 1] - start
        alive = alive & (deg > 0)
        pos = start + th.minimum((th.rand(n, device=seeds.device) * deg).long(), (deg - 1).clamp(min=0))
        nxt = indices[th.where(alive, pos, th.zeros_like(pos))].long()
        cur = th.where(alive, nxt, th.full_like(nxt, -1))
        cols.append(cur)
        if probs is not None and probs[t] > 0:
            alive = alive & (th.rand(n, device=seeds.device) >= probs[t])
    return th.stack(cols, 1)


def torch_visit_topk(traces, walks_per_seed, col0, col_step, k, num_nodes):
    cand = traces[:, col0::col_step]
    slot = (th.arange(traces.shape[0], device=traces.device) // walks_per_seed).unsqueeze(1)
    valid = cand >= 0
    keys = (slot * num_nodes + cand)[valid]
    uniq, cnt = th.unique(keys, return_counts=True)  # ascending: by slot, then by id
    s, ids = uniq // num_nodes, uniq % num_nodes
    by_count = th.argsort(cnt, descending=True, stable=True)
    order = by_count[th.argsort(s[by_count], stable=True)]
    s, ids, cnt = s[order], ids[order], cnt[order]
    num_slots = traces.shape[0] // walks_per_seed
    per_slot = th.bincount(s, minlength=num_slots)
    first = th.cumsum(per_slot, 0) - per_slot
    keep = th.arange(s.shape[0], device=s.device) - first[s] < k
    return ids[keep], s[keep], cnt[keep]


def walk_record(csrs, tcsrs, path, seeds, thr, probs, window_ms, rounds):
    dev = seeds.device
    pt = th.tensor(path, dtype=th.int32).to(dev)
    tt = None if thr is None else th.tensor(thr, dtype=th.int64).to(dev)
    run = lambda variant: K.random_walk(csrs, pt, seeds, tt, 1, variant=variant)
    plain, staged, torch_side = compare(
        [lambda: run(1), lambda: run(2), lambda: torch_walk(tcsrs, path, seeds, probs)],
        window_ms, rounds)
    a, b = run(1), run(2)
    found = int((a[:, 1:] >= 0).sum())
    alive_before = int((a[:, :-1] >= 0).sum())  # an upper bound of the steps attempted
    rec = {"walks": int(seeds.shape[0]), "length": len(path),
           "plain_stores": plain, "staged_stores": staged, "torch_ops": torch_side,
           "variants_same_bits": bool(th.equal(a, b)),
           "plain_over_staged": plain["ms"] / staged["ms"],
           "staged_below_plain_by_more_than_spread": spread_gate(staged, plain),
           "plain_below_staged_by_more_than_spread": spread_gate(plain, staged),
           "steps_that_found_an_edge": found, "steps_attempted_at_most": alive_before,
           "trace_bytes": int(a.numel() * 8)}
    for name, side in (("plain", plain), ("staged", staged)):
        rec["torch_over_" + name] = torch_side["ms"] / side["ms"]
        rec[name + "_steps_per_s"] = found / (side["ms"] * 1e-3)
        rec[name + "_dependent_loads_per_s"] = 2 * found / (side["ms"] * 1e-3)
        rec[name + "_below_torch_by_more_than_spread"] = spread_gate(side, torch_side)
    return rec, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "randomwalk_bench.json"))
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=int, default=20, help="log2 of the node counts' unit")
    ap.add_argument("--edges", type=int, default=16 * 2 ** 20)
    ap.add_argument("--seeds", type=int, default=4096)
    args = ap.parse_args()
    if not th.cuda.is_available():
        raise SystemExit("bench_randomwalk needs the GPU: nothing is timed without one")
    dev = th.device("cuda:0")
    th.manual_seed(0)
    res = {"device": th.cuda.get_device_name(0),
           "timing": "device events around windows of about %g ms of calls, median (and min, "
                     "max) of %d alternating windows" % (args.window_ms, args.rounds),
           "stage_chunk_columns": K.walk_stage_chunk()}

    # ---- PinSAGE ---------------------------------------------------------------------
    nu, ni, m = 2 ** args.scale, 2 ** (args.scale - 2), args.edges
    users = chung_lu_edges(nu, m, 0.6, 1, dev)[0]
    items = chung_lu_edges(ni, m, 0.8, 2, dev)[1]
    ui = device_block_gidx(nu, ni, users, items).out_csr
    iu = device_block_gidx(ni, nu, items, users).out_csr
    csrs = [iu, ui]                                  # item -> user -> item
    tcsrs = [(c.indptr.long(), c.indices) for c in csrs]
    walks, rounds_, hops, k = 200, 3, 2, 10
    path = [0, 1] * rounds_
    probs = [0.0] * len(path)
    for t in range(hops, len(path), hops):
        probs[t] = 0.5
    thr = K.restart_thresholds(probs)
    deg = iu.indptr[1:] - iu.indptr[:-1]
    seeds = th.nonzero(deg > 0).reshape(-1)
    seeds = seeds[th.randperm(seeds.shape[0], device=dev)[:args.seeds]].int()
    rep = seeds.repeat_interleave(walks)
    rec, traces = walk_record(csrs, tcsrs, path, rep, thr, probs, args.window_ms, args.rounds)
    ours, theirs = compare(
        [lambda: K.visit_topk(traces, walks, hops, hops, k),
         lambda: torch_visit_topk(traces, walks, hops, hops, k, ni)], args.window_ms, args.rounds)
    nbr, cnt, num = K.visit_topk(traces, walks, hops, hops, k)
    t_ids, t_slot, t_cnt = torch_visit_topk(traces, walks, hops, hops, k, ni)
    keep = nbr >= 0
    res["pinsage"] = {
        "graph": {"users": nu, "items": ni, "edges_per_direction": m,
                  "max_item_degree": int(deg.max())},
        "seeds": int(seeds.shape[0]), "walks_per_seed": walks, "traversals": rounds_, "hops": hops,
        "restart": 0.5, "k": k, "walk": rec,
        "visit_topk": ours, "torch_unique_sort_topk": theirs,
        "torch_over_visit_topk": theirs["ms"] / ours["ms"],
        "visit_topk_below_torch_by_more_than_spread": spread_gate(ours, theirs),
        "visit_tile": list(K.visit_tile(walks * rounds_, k)),
        "same_as_torch": bool(th.equal(nbr[keep].long(), t_ids) and th.equal(cnt[keep].long(), t_cnt)),
        "edges": int(keep.sum())}
    print("pinsage", json.dumps(res["pinsage"]), flush=True)
    del traces, rep

    # ---- DeepWalk --------------------------------------------------------------------
    n = 2 ** args.scale
    s, d = chung_lu_edges(n, m, 0.6, 3, dev)
    sym = device_block_gidx(n, n, th.cat([s, d]), th.cat([d, s])).out_csr
    L = 40
    starts = th.randint(0, n, (2 ** 20,), device=dev, dtype=th.int32)
    rec, _ = walk_record([sym], [(sym.indptr.long(), sym.indices)], [0] * L, starts, None, None,
                         args.window_ms, args.rounds)
    res["deepwalk"] = {"graph": {"nodes": n, "edges": 2 * m,
                                 "max_degree": int((sym.indptr[1:] - sym.indptr[:-1]).max())},
                       "walk": rec}
    print("deepwalk", json.dumps(res["deepwalk"]), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"wrote": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
