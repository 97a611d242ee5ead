"""PinSAGE neighbour sampling and one weighted aggregation, everything on one GPU.

A synthetic user-item graph of 8 clusters without a single edge between clusters, both
directions as relations.  ``dgl.sampling.PinSAGESampler`` picks, for every item of a batch,
the items its random walks with restarts visit most; ``dgl.to_block`` compacts the frontier;
one ``u_mul_e`` / ``sum`` pass aggregates the neighbours' features weighted by the visit counts
normalised per seed, and is compared with ``torch.index_add_``.

Because the clusters are disconnected, a walk never leaves its seed's cluster: the example
asserts that every sampled neighbour lies in its seed's cluster -- exactly, not as a share --
then prints a line ending in ``ok``.  No node id visits the host inside a batch.

    python examples/pinsage_sampling.py
"""
import argparse
import os
import sys
import time

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "dgl-hack_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import dgl  # noqa: E402
import dgl.function as fn  # noqa: E402

CLUSTERS = 8


def cluster_graph(users, items, views, rng):
    """``users`` / ``items`` per cluster; every user views ``views`` items of its own cluster.
    Returns (user ids, item ids) of the view edges and the items' clusters."""
    u = np.repeat(np.arange(CLUSTERS * users), views)
    i = (u // users) * items + rng.integers(0, items, u.shape[0])
    return u, i, np.arange(CLUSTERS * items) // items


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=60, help="per cluster")
    ap.add_argument("--items", type=int, default=40, help="per cluster")
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--neighbors", type=int, default=10)
    args = ap.parse_args()
    dev = th.device("cuda:0")
    th.manual_seed(0)
    rng = np.random.default_rng(0)
    u, i, item_cluster = cluster_graph(args.users, args.items, 5, rng)
    n_users, n_items = CLUSTERS * args.users, CLUSTERS * args.items
    G = dgl.heterograph({("user", "viewed", "item"): (u, i), ("item", "viewed-by", "user"): (i, u)},
                        num_nodes_dict={"user": n_users, "item": n_items})
    sampler = dgl.sampling.PinSAGESampler(G, "item", "user", 3, 0.5, 200, args.neighbors)
    x = th.randn(n_items, 32, device=dev)
    cluster = th.from_numpy(item_cluster).to(dev)

    t0 = time.time()
    edges, batches = 0, 0
    order = th.randperm(n_items).to(dev)
    for start in range(0, n_items, args.batch_size):
        seeds = order[start:start + args.batch_size]
        frontier = sampler(seeds)
        assert frontier.number_of_nodes() == n_items
        block = dgl.to_block(frontier, seeds)
        src_local, dst_local = block._graph.device_uv(dev)  # block ids, edge by edge
        src = block.srcdata[dgl.NID][src_local]             # global ids
        dst = block.dstdata[dgl.NID][dst_local]
        # the condition the disconnected clusters impose: no neighbour outside the seed's
        assert bool((cluster[src] == cluster[dst]).all()), "a walk left its cluster"
        assert th.equal(block.dstdata[dgl.NID], seeds)

        counts = frontier.edata["weights"][block.edata[dgl.EID]].float()
        total = th.zeros(seeds.shape[0], device=dev).index_add_(0, dst_local, counts)
        w = (counts / total[dst_local]).unsqueeze(1)
        block.srcdata["h"] = x[block.srcdata[dgl.NID]]
        block.edata["w"] = w
        block.update_all(fn.u_mul_e("h", "w", "m"), fn.sum("m", "y"))
        got = block.dstdata["y"]
        want = th.zeros(seeds.shape[0], x.shape[1], device=dev).index_add_(0, dst_local, x[src] * w)
        assert th.allclose(got, want, rtol=1e-4, atol=1e-5), float((got - want).abs().max())
        edges += int(src.shape[0])
        batches += 1
    th.cuda.synchronize()
    assert edges > 0
    print("batches %d  items %d  sampled edges %d  every neighbour in its seed's cluster  %.1f s  ok"
          % (batches, n_items, edges, time.time() - t0))


if __name__ == "__main__":
    main()
