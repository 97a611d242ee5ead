#!/usr/bin/env python3
"""Point-cloud classification in the shape of DGCNN (Wang et al., "Dynamic Graph CNN for
Learning on Point Clouds"; the reference's examples/pytorch/pointcloud/model.py), on one
MI355X: k-NN graph -> EdgeConv -> k-NN graph rebuilt in FEATURE space -> EdgeConv ->
MaxPooling -> Linear.  The graph is rebuilt inside every training step, which is why its
construction is a device kernel (``dgl.kernel.knn_select``) here.

The set is synthetic and generated in numpy: class 0 are points on a sphere's surface,
class 1 points on a cube's surface, class 2 two Gaussian blobs; every cloud is jittered
and has its own number of points (40 to 80), so the clouds are stored one after another
and ``SegmentedKNNGraph`` builds the batch.  The graph it returns carries the clouds' sizes
as batch information, which is all ``MaxPooling`` needs for one vector per cloud.  Seeds
are fixed; the losses are printed and the last line is a JSON record.

  python examples/dgcnn_pointcloud.py [--steps 60] [--clouds 90] [--k 8]

tests/test_knn_gpu.py asks of the default run that the last loss is below the first and
that at least 90 % of the set is classified; the run reaches 100 % on its fixed seed.
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


def make_set(num_clouds, seed):
    """points (N, 3) float32, the clouds' sizes, labels."""
    rng = np.random.default_rng(seed)
    pts, segs, labels = [], [], []
    for i in range(num_clouds):
        m = int(rng.integers(40, 81))
        label = i % 3
        if label == 0:
            p = rng.standard_normal((m, 3))
            p /= np.linalg.norm(p, axis=1, keepdims=True)
        elif label == 1:
            p = rng.uniform(-1, 1, (m, 3))
            p[np.arange(m), rng.integers(0, 3, m)] = rng.choice([-1.0, 1.0], m)
        else:
            c = np.where(rng.random((m, 1)) < 0.5, -0.6, 0.6) * np.ones((1, 3))
            p = c + 0.2 * rng.standard_normal((m, 3))
        p = p + 0.02 * rng.standard_normal((m, 3))
        pts.append(p.astype(np.float32))
        segs.append(m)
        labels.append(label)
    return np.concatenate(pts), segs, np.asarray(labels, np.int64)


class DGCNN(nn.Module):
    def __init__(self, k, hidden, classes):
        super(DGCNN, self).__init__()
        from dgl.nn.pytorch import EdgeConv, MaxPooling, SegmentedKNNGraph
        self.nng = SegmentedKNNGraph(k)
        self.conv1 = EdgeConv(3, hidden)
        self.conv2 = EdgeConv(hidden, 2 * hidden)
        self.pool = MaxPooling()
        self.out = nn.Linear(2 * hidden, classes)

    def forward(self, x, segs):
        g = self.nng(x, segs)
        h = F.leaky_relu(self.conv1(g, x), 0.2)
        g = self.nng(h, segs)  # neighbours in feature space
        h = F.leaky_relu(self.conv2(g, h), 0.2)
        return self.out(self.pool(g, h))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--clouds", type=int, default=90)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--lr", type=float, default=0.01)
    args = ap.parse_args()

    pts, segs, labels = make_set(args.clouds, 0)
    dev = th.device("cuda:0")
    th.manual_seed(0)
    model = DGCNN(args.k, args.hidden, 3).to(dev)
    x = th.from_numpy(pts).to(dev)
    y = th.from_numpy(labels).to(dev)

    opt = th.optim.Adam(model.parameters(), lr=args.lr)
    losses = []
    for step in range(args.steps):
        loss = F.cross_entropy(model(x, segs), y)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
        print("step %3d  loss %.4f" % (step, losses[-1]))
    with th.no_grad():
        acc = float((model(x, segs).argmax(1) == y).float().mean())
    print(json.dumps({"first_loss": losses[0], "last_loss": losses[-1], "train_acc": acc,
                      "steps": args.steps, "clouds": args.clouds, "points": int(x.shape[0]),
                      "k": args.k, "form": "dgl on " + str(y.device)}))


if __name__ == "__main__":
    main()
