"""Minibatch GraphSAGE with neighbour sampling, everything on one GPU.

The single-GPU path of the reference's ``examples/pytorch/graphsage/train_sampling.py`` on a
synthetic community graph: per minibatch, ``dgl.sampling.sample_neighbors`` draws a fan-out
of in-neighbours layer by layer, ``dgl.to_block`` compacts each frontier into a bipartite
block, and a two-layer SAGE runs over the blocks on ``x[input_nodes]`` gathered on the
device.  Evaluation infers layer by layer over all nodes through ``dgl.in_subgraph`` +
``dgl.to_block``.  No node or edge id visits the host inside a step.

Asserts that the loss falls and that the final accuracy is above the majority-class rate,
then prints a line ending in ``ok``.

    python examples/graphsage_sampling.py
"""
import argparse
import os
import sys
import time

import numpy as np
import torch as th
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "dgl-hack_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import dgl  # noqa: E402
from dgl.nn.pytorch import SAGEConv  # noqa: E402


def community_graph(n, classes, degree, p_in, rng):
    """Nodes in ``classes`` communities of unequal size; each node draws ``degree``
    in-neighbours, a fraction ``p_in`` of them from its own community.  Features are the
    community's direction buried in noise, so a node alone is a weak predictor and its
    neighbourhood a good one."""
    share = np.arange(classes, 0, -1, dtype=np.float64)
    labels = rng.choice(classes, n, p=share / share.sum())
    members = [np.nonzero(labels == c)[0] for c in range(classes)]
    dst = np.repeat(np.arange(n), degree)
    own = rng.random(n * degree) < p_in
    src = rng.integers(0, n, n * degree)
    for c in range(classes):
        sel = own & (labels[dst] == c)
        src[sel] = rng.choice(members[c], int(sel.sum()))
    feats = rng.normal(0, 1, (n, 16)).astype(np.float32)
    feats[np.arange(n), labels] += 0.6
    return src, dst, feats, labels


class NeighborSampler:
    def __init__(self, g, fanouts):
        self.g, self.fanouts = g, fanouts

    def sample_blocks(self, seeds):
        blocks = []
        for fanout in self.fanouts:
            frontier = dgl.sampling.sample_neighbors(self.g, seeds, fanout, replace=True)
            block = dgl.to_block(frontier, seeds)
            seeds = block.srcdata[dgl.NID]  # the next layer's seeds, on the device
            blocks.insert(0, block)
        return blocks


class SAGE(nn.Module):
    def __init__(self, in_feats, hidden, classes, dropout):
        super().__init__()
        self.hidden, self.classes = hidden, classes
        self.layers = nn.ModuleList([SAGEConv(in_feats, hidden, "mean"),
                                     SAGEConv(hidden, classes, "mean")])
        self.dropout = nn.Dropout(dropout)

    def forward(self, blocks, x):
        h = x
        for i, (layer, block) in enumerate(zip(self.layers, blocks)):
            h = layer(block, (h, h[:block.number_of_dst_nodes()]))
            if i + 1 < len(self.layers):
                h = self.dropout(F.relu(h))
        return h

    def inference(self, g, x, batch_size):
        """All nodes, layer by layer, over every in-edge (no sampling)."""
        n = g.number_of_nodes()
        nodes = th.arange(n, device=x.device)
        for i, layer in enumerate(self.layers):
            y = x.new_zeros(n, self.hidden if i + 1 < len(self.layers) else self.classes)
            for start in range(0, n, batch_size):
                batch = nodes[start:start + batch_size]
                block = dgl.to_block(dgl.in_subgraph(g, batch), batch)
                h = x[block.srcdata[dgl.NID]]
                h = layer(block, (h, h[:block.number_of_dst_nodes()]))
                y[start:start + batch_size] = F.relu(h) if i + 1 < len(self.layers) else h
            x = y
        return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=6000)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--batch-size", type=int, default=500)
    ap.add_argument("--fanouts", type=str, default="10,25")
    args = ap.parse_args()
    dev = th.device("cuda:0")
    th.manual_seed(0)
    rng = np.random.default_rng(0)
    classes = 5
    src, dst, feats, labels = community_graph(args.nodes, classes, 12, 0.7, rng)
    g = dgl.DGLGraph.from_device_coo(th.from_numpy(src.astype(np.int32)).to(dev),
                                     th.from_numpy(dst.astype(np.int32)).to(dev), args.nodes)
    x = th.from_numpy(feats).to(dev)
    y = th.from_numpy(labels).to(dev)
    train = th.from_numpy(rng.permutation(args.nodes)[:args.nodes // 2]).to(dev)
    test_mask = th.ones(args.nodes, dtype=th.bool, device=dev)
    test_mask[train] = False

    sampler = NeighborSampler(g, [int(f) for f in args.fanouts.split(",")])
    model = SAGE(feats.shape[1], 32, classes, 0.2).to(dev)
    opt = th.optim.Adam(model.parameters(), lr=0.01)
    losses = []
    t0 = time.time()
    for epoch in range(args.epochs):
        order = train[th.randperm(train.shape[0], device=dev)]
        total, steps = 0.0, 0
        for start in range(0, order.shape[0], args.batch_size):
            seeds = order[start:start + args.batch_size]
            blocks = sampler.sample_blocks(seeds)
            input_nodes = blocks[0].srcdata[dgl.NID]
            loss = F.cross_entropy(model(blocks, x[input_nodes]), y[seeds])
            opt.zero_grad()
            loss.backward()
            opt.step()
            total += float(loss.detach())
            steps += 1
        losses.append(total / steps)
    model.eval()
    with th.no_grad():
        pred = model.inference(g, x, 2000).argmax(1)
    acc = float((pred[test_mask] == y[test_mask]).float().mean())
    majority = float(np.bincount(labels).max()) / args.nodes
    th.cuda.synchronize()
    assert losses[-1] < losses[0], losses
    assert acc > majority + 0.05, (acc, majority)
    print("epochs %d  loss %.3f -> %.3f  test acc %.3f (majority class %.3f)  %.1f s  ok"
          % (args.epochs, losses[0], losses[-1], acc, majority, time.time() - t0))


if __name__ == "__main__":
    main()
