"""Cluster-GCN on one GPU: every step trains on the subgraph induced on a few clusters.

The training loop of Cluster-GCN (Chiang et al., KDD 2019) on a synthetic graph of planted
clusters (``dgl.data.synthetic.planted_cluster_edges``, clusters = the planted labels' parts):
per step, ``g.subgraph(union of q clusters)`` cuts the induced subgraph on the device,
``copy_from_parent()`` gathers its features and labels, and two ``GraphConv`` layers run on it.
No node or edge id visits the host inside a step.

Asserts that the loss falls and that every subgraph edge has both ends in the chosen
clusters, then prints a line ending in ``ok``.

    python examples/cluster_gcn.py
"""
import argparse
import os
import sys
import time

import torch as th
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "dgl-hack_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import dgl  # noqa: E402
from dgl.data.synthetic import planted_cluster_edges  # noqa: E402
from dgl.nn.pytorch import GraphConv  # noqa: E402


class GCN(nn.Module):
    def __init__(self, in_feats, hidden, classes):
        super().__init__()
        self.l1 = GraphConv(in_feats, hidden, norm="right", activation=F.relu)
        self.l2 = GraphConv(hidden, classes, norm="right")

    def forward(self, g, x):
        return self.l2(g, self.l1(g, x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=20000)
    ap.add_argument("--clusters", type=int, default=40)
    ap.add_argument("--classes", type=int, default=5)
    ap.add_argument("--degree", type=int, default=10)
    ap.add_argument("--q", type=int, default=4, help="clusters per step")
    ap.add_argument("--steps", type=int, default=40)
    args = ap.parse_args()
    dev = th.device("cuda:0")
    th.manual_seed(0)
    n, k = args.nodes, args.clusters

    src, dst, part = planted_cluster_edges(n, k, n * args.degree, 0.8, 0, dev)
    loops = th.arange(n, dtype=th.int32, device=dev)  # every node keeps an in-edge in any cut
    src, dst = th.cat([src, loops]), th.cat([dst, loops])
    g = dgl.DGLGraph.from_device_coo(src, dst, n)
    label = part % args.classes
    x = th.randn(n, 16, device=dev)
    x[th.arange(n, device=dev), label] += 0.5  # a weak signal per node, a clear one per cluster
    g.ndata["x"], g.ndata["y"], g.ndata["part"] = x, label, part

    model = GCN(16, 32, args.classes).to(dev)
    opt = th.optim.Adam(model.parameters(), lr=0.02)
    gen = th.Generator().manual_seed(1)
    losses, edges = [], 0
    t0 = time.time()
    for _ in range(args.steps):
        chosen = th.randperm(k, generator=gen)[:args.q].to(dev)
        member = th.zeros(k, dtype=th.bool, device=dev)
        member[chosen] = True
        sg = g.subgraph(th.nonzero(member[part]).reshape(-1))
        sg.copy_from_parent()
        ends = th.cat([src[sg.parent_eid], dst[sg.parent_eid]]).long()  # in the parent's ids
        assert bool(member[part[ends]].all()), "a subgraph edge leaves the chosen clusters"
        assert th.equal(sg.ndata["part"], part[sg.parent_nid])
        edges += sg.number_of_edges()
        loss = F.cross_entropy(model(sg, sg.ndata["x"]), sg.ndata["y"])
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    th.cuda.synchronize()
    first, last = sum(losses[:5]) / 5, sum(losses[-5:]) / 5
    assert last < 0.7 * first, "the loss did not fall: %.3f -> %.3f" % (first, last)
    print("loss %.3f -> %.3f, %d subgraph edges per step, %.2f s: cluster_gcn ok"
          % (first, last, edges // args.steps, time.time() - t0))


if __name__ == "__main__":
    main()
