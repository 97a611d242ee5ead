#!/usr/bin/env python3
"""Graph classification on a batch of small graphs: GINConv x 2 -> SumPooling -> Linear
(the shape of the reference's examples/pytorch/gin), on one MI355X.

The set is synthetic and generated in numpy: class 0 are cycles, class 1 are stars, 8 to 20
nodes each, every graph with up to two random extra edges, all edges in both directions;
every node's input feature is 1.  The whole set is one ``dgl.batch``; each step is a full
pass: two GIN layers over the batched graph, one vector per graph from ``SumPooling`` (the
segment-sum kernel), cross entropy, Adam.  Seeds are fixed; the losses are printed and the
last line is a JSON record.

  python examples/gin_graph_classify.py [--steps 60] [--graphs 200]
  python examples/gin_graph_classify.py --restate    # the same model in float64 torch, CPU

``--restate`` runs the same model, initial weights and data as dense float64 torch
operations on the CPU (adjacency and segment matrices, no kernel of this package).  The
default of 60 steps was picked with it: the restatement's last loss is below its first and
it classifies at least 90 % of the set, which is what tests/test_glob_gpu.py asks of the
device run.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "dgl-hack_amd"), os.path.join(ROOT, "examples")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch as th  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def make_set(num_graphs, seed):
    """[(num_nodes, src, dst)], labels: cycles (0) and stars (1) with random extra edges."""
    rng = np.random.default_rng(seed)
    graphs, labels = [], []
    for i in range(num_graphs):
        n = int(rng.integers(8, 21))
        label = i % 2
        if label == 0:
            u = np.arange(n)
            v = (u + 1) % n
        else:
            u = np.zeros(n - 1, np.int64)
            v = np.arange(1, n)
        extra = int(rng.integers(0, 3))
        u = np.concatenate([u, rng.integers(0, n, extra)])
        v = np.concatenate([v, rng.integers(0, n, extra)])
        graphs.append((n, np.concatenate([u, v]), np.concatenate([v, u])))
        labels.append(label)
    return graphs, np.asarray(labels, np.int64)


def mlp(i, o):
    return nn.Sequential(nn.Linear(i, o), nn.ReLU(), nn.Linear(o, o))


class GIN(nn.Module):
    def __init__(self, hidden, classes):
        super(GIN, self).__init__()
        from dgl.nn.pytorch import GINConv, SumPooling
        self.conv1 = GINConv(mlp(1, hidden), "sum")
        self.conv2 = GINConv(mlp(hidden, hidden), "sum")
        self.pool = SumPooling()
        self.out = nn.Linear(hidden, classes)

    def forward(self, g, x):
        h = F.relu(self.conv1(g, x))
        h = F.relu(self.conv2(g, h))
        return self.out(self.pool(g, h))


class DenseGIN(nn.Module):
    """The same model on a dense adjacency A (dst x src) and a segment matrix P (graphs x
    nodes): GIN's sum aggregation is A h + (1 + eps) h with eps = 0, the pooling P h."""

    def __init__(self, hidden, classes):
        super(DenseGIN, self).__init__()
        self.mlp1, self.mlp2 = mlp(1, hidden), mlp(hidden, hidden)
        self.out = nn.Linear(hidden, classes)

    def forward(self, A, P, x):
        h = F.relu(self.mlp1(A @ x + x))
        h = F.relu(self.mlp2(A @ h + h))
        return self.out(P @ h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--graphs", type=int, default=200)
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--restate", action="store_true")
    args = ap.parse_args()

    graphs, labels = make_set(args.graphs, 0)
    th.manual_seed(0)
    dense = DenseGIN(args.hidden, 2)  # the initial weights of both forms
    if args.restate:
        n = sum(g[0] for g in graphs)
        A = th.zeros(n, n, dtype=th.float64)
        P = th.zeros(len(graphs), n, dtype=th.float64)
        off = 0
        for b, (k, s, d) in enumerate(graphs):
            A.index_put_((th.from_numpy(d + off), th.from_numpy(s + off)),
                         th.ones(len(s), dtype=th.float64), accumulate=True)
            P[b, off:off + k] = 1
            off += k
        model = dense.double()
        x, y = th.ones(n, 1, dtype=th.float64), th.from_numpy(labels)
        run = lambda: model(A, P, x)
    else:
        import dgl
        dev = th.device("cuda:0")
        gs = []
        for k, s, d in graphs:
            g = dgl.DGLGraph()
            g.add_nodes(k)
            g.add_edges(s, d)
            gs.append(g)
        bg = dgl.batch(gs)
        model = GIN(args.hidden, 2)
        model.conv1.apply_func.load_state_dict(dense.mlp1.state_dict())
        model.conv2.apply_func.load_state_dict(dense.mlp2.state_dict())
        model.out.load_state_dict(dense.out.state_dict())
        model = model.to(dev)
        x = th.ones(bg.number_of_nodes(), 1, device=dev)
        y = th.from_numpy(labels).to(dev)
        run = lambda: model(bg, x)

    opt = th.optim.Adam(model.parameters(), lr=args.lr)
    losses = []
    for step in range(args.steps):
        loss = F.cross_entropy(run(), y)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
        print("step %3d  loss %.4f" % (step, losses[-1]))
    with th.no_grad():
        acc = float((run().argmax(1) == y).float().mean())
    print(json.dumps({"first_loss": losses[0], "last_loss": losses[-1], "train_acc": acc,
                      "steps": args.steps, "graphs": args.graphs,
                      "form": "float64 dense torch" if args.restate else "dgl on " + str(y.device)}))


if __name__ == "__main__":
    main()
