"""Child-sum TreeLSTM (Tai et al., 2015) on a batch of synthetic random trees, swept bottom-up
by ``dgl.prop_nodes_topo``: the topological frontiers come from the device traversal kernels,
each frontier pulls the sum of its children's states (``copy_u`` / ``sum``) and the cell runs
as the apply function.  The forget gate of the child-sum cell depends on the child alone, so
a child sends ``[h, f * c]`` and the parent needs nothing but the sum.

The task: regress, at every root, the mean of the first input feature over its tree.
Prints one JSON line with the first and the last training loss.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch as th
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "dgl-hack_amd"))
import dgl  # noqa: E402
import dgl.function as fn  # noqa: E402


class ChildSumCell(nn.Module):
    def __init__(self, x_size, h_size):
        super().__init__()
        self.h_size = h_size
        self.w_iou = nn.Linear(x_size, 3 * h_size)
        self.u_iou = nn.Linear(h_size, 3 * h_size, bias=False)
        self.u_f = nn.Linear(h_size, h_size)

    def forward(self, nodes):
        h_sum, fc_sum = nodes.data["acc"].split(self.h_size, 1)  # zeros at the leaves
        i, o, u = (self.w_iou(nodes.data["x"]) + self.u_iou(h_sum)).chunk(3, 1)
        c = th.sigmoid(i) * th.tanh(u) + fc_sum
        h = th.sigmoid(o) * th.tanh(c)
        return {"h": h, "hc": th.cat([h, th.sigmoid(self.u_f(h)) * c], 1)}


class TreeLSTM(nn.Module):
    def __init__(self, x_size, h_size):
        super().__init__()
        self.cell = ChildSumCell(x_size, h_size)
        self.out = nn.Linear(h_size, 1)

    def forward(self, g, x, roots):
        n, h = g.number_of_nodes(), self.cell.h_size
        g.ndata["x"] = x
        g.ndata["acc"] = x.new_zeros(n, 2 * h)
        g.ndata["hc"] = x.new_zeros(n, 2 * h)
        g.ndata["h"] = x.new_zeros(n, h)  # fresh columns: nothing of the last step's graph stays
        dgl.prop_nodes_topo(g, message_func=fn.copy_u("hc", "m"), reduce_func=fn.sum("m", "acc"),
                            apply_node_func=self.cell)
        return self.out(g.ndata["h"][roots]).squeeze(1)


def random_trees(rng, count, max_nodes):
    """Trees with edges child -> parent; node 0 of every tree is its root."""
    trees = []
    for _ in range(count):
        n = int(rng.integers(2, max_nodes + 1))
        t = dgl.DGLGraph()
        t.add_nodes(n)
        t.add_edges(np.arange(1, n), [int(rng.integers(max(0, c - 3), c)) for c in range(1, n)])
        trees.append(t)
    return trees


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--trees", type=int, default=16)
    ap.add_argument("--max-nodes", type=int, default=24)
    ap.add_argument("--hidden", type=int, default=16)
    args = ap.parse_args()
    th.manual_seed(0)
    rng = np.random.default_rng(0)
    dev = th.device("cuda:0")
    trees = random_trees(rng, args.trees, args.max_nodes)
    sizes = np.array([t.number_of_nodes() for t in trees])
    g = dgl.batch(trees)
    roots = th.from_numpy(np.cumsum(sizes) - sizes).to(dev)
    x = th.from_numpy(rng.normal(size=(int(sizes.sum()), 4)).astype(np.float32)).to(dev)
    tree_of = th.from_numpy(np.repeat(np.arange(len(sizes)), sizes)).to(dev)
    target = th.zeros(len(sizes), device=dev).index_add_(0, tree_of, x[:, 0]) / th.from_numpy(
        sizes.astype(np.float32)).to(dev)
    model = TreeLSTM(4, args.hidden).to(dev)
    opt = th.optim.Adam(model.parameters(), lr=0.02)
    losses = []
    for _ in range(args.steps):
        loss = ((model(g, x, roots) - target) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print(json.dumps({"loss_first": losses[0], "loss_last": losses[-1], "steps": args.steps,
                      "nodes": int(sizes.sum())}))


if __name__ == "__main__":
    main()
