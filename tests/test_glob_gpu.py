"""dgl.nn.pytorch.glob on the GPU: each pooling module against a float64 torch restatement
computed graph by graph, on a batch of five graphs of 1, 7, 64, 0 and 200 nodes at F = 32
(the graphs of 1 and 0 nodes exercise SortPooling's padding and the empty segment).
Forward, input gradient and parameter gradients at rtol 1e-4 / atol 1e-5, the module-level
bounds of test_nn_gpu.py.  State-dict keys are the reference's, and the graph
classification example trains."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as th
import torch.nn as nn

import dgl
from dgl.nn.pytorch import (SumPooling, AvgPooling, MaxPooling, SortPooling,
                            GlobalAttentionPooling, Set2Set, WeightAndSum)

pytestmark = pytest.mark.gpu
DEV = th.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 7, 64, 0, 200]
F = 32
K_SORT = 10


def _batch():
    gs = []
    for i, n in enumerate(SIZES):
        g = dgl.DGLGraph()
        g.add_nodes(n)
        if n > 1:
            rng = np.random.default_rng(i)
            g.add_edges(rng.integers(0, n, 2 * n), rng.integers(0, n, 2 * n))
        gs.append(g)
    return dgl.batch(gs)


# ---- float64 restatements, one graph's rows at a time ----------------------------------------
def _ref_sum(m, xs):
    return th.stack([x.sum(0) for x in xs])


def _ref_avg(m, xs):
    return th.stack([x.mean(0) if len(x) else x.new_zeros(F) for x in xs])


def _ref_max(m, xs):
    return th.stack([x.max(0)[0] if len(x) else x.new_full((F,), -float("inf")) for x in xs])


def _ref_sort(m, xs):
    out = []
    for x in xs:
        s = x.sort(-1)[0]
        top = s[th.argsort(s[:, -1], descending=True)[:K_SORT]]
        out.append(th.cat([top, x.new_zeros(K_SORT - len(top), F)]).reshape(-1))
    return th.stack(out)


def _ref_attn(m, xs):
    out = []
    for x in xs:
        gate = th.softmax(m.gate_nn(x), 0)
        feat = m.feat_nn(x) if m.feat_nn is not None else x
        out.append((feat * gate).sum(0))
    return th.stack(out)


def _ref_set2set(m, xs):
    b = len(xs)
    h = (xs[0].new_zeros((m.n_layers, b, m.input_dim)), xs[0].new_zeros((m.n_layers, b, m.input_dim)))
    q_star = xs[0].new_zeros(b, m.output_dim)
    for _ in range(m.n_iters):
        q, h = m.lstm(q_star.unsqueeze(0), h)
        q = q.view(b, m.input_dim)
        reads = []
        for i, x in enumerate(xs):
            alpha = th.softmax((x * q[i]).sum(-1, keepdim=True), 0)
            reads.append((x * alpha).sum(0))
        q_star = th.cat([q, th.stack(reads)], -1)
    return q_star


def _ref_weight_and_sum(m, xs):
    return th.stack([(x * m.atom_weighting(x)).sum(0) for x in xs])


MODULES = {
    "sum": (lambda: SumPooling(), _ref_sum),
    "avg": (lambda: AvgPooling(), _ref_avg),
    "max": (lambda: MaxPooling(), _ref_max),
    "sort": (lambda: SortPooling(k=K_SORT), _ref_sort),
    "attention": (lambda: GlobalAttentionPooling(nn.Linear(F, 1), nn.Linear(F, F)), _ref_attn),
    "set2set": (lambda: Set2Set(F, n_iters=3, n_layers=1), _ref_set2set),
    "weight_and_sum": (lambda: WeightAndSum(F), _ref_weight_and_sum),
}


@pytest.mark.parametrize("name", list(MODULES))
def test_module_matches_float64_restatement(name):
    make, ref = MODULES[name]
    bg = _batch()
    th.manual_seed(3)
    mod = make()
    mod64 = copy.deepcopy(mod).double()
    mod = mod.to(DEV)
    n = sum(SIZES)
    x = th.randn(n, F)
    xg = x.to(DEV).requires_grad_()
    out = mod(bg, xg)
    x64 = x.double().requires_grad_()
    want = ref(mod64, list(th.split(x64, SIZES)))
    assert out.shape == want.shape
    assert th.allclose(out.detach().cpu().double(), want.detach(), rtol=1e-4, atol=1e-5)
    gy = th.randn(out.shape)
    params, params64 = list(mod.parameters()), list(mod64.parameters())
    grads = th.autograd.grad(out, [xg] + params, gy.to(DEV))
    grads64 = th.autograd.grad(want, [x64] + params64, gy.double())
    assert len(grads) == len(grads64)
    for g, g64 in zip(grads, grads64):
        assert th.allclose(g.cpu().double(), g64, rtol=1e-4, atol=1e-5), (g.cpu().double() - g64).abs().max()


def test_state_dict_keys_are_the_references():
    keys = {name: sorted(make().state_dict().keys()) for name, (make, _) in MODULES.items()}
    assert keys == {
        "sum": [], "avg": [], "max": [], "sort": [],
        "attention": ["feat_nn.bias", "feat_nn.weight", "gate_nn.bias", "gate_nn.weight"],
        "set2set": ["lstm.bias_hh_l0", "lstm.bias_ih_l0", "lstm.weight_hh_l0", "lstm.weight_ih_l0"],
        "weight_and_sum": ["atom_weighting.0.bias", "atom_weighting.0.weight"],
    }


def test_gin_graph_classification_example_trains():
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "examples", "gin_graph_classify.py")],
                                  timeout=300)
    r = json.loads(out.decode().strip().splitlines()[-1])
    assert r["last_loss"] < r["first_loss"], r
    assert r["train_acc"] >= 0.9, r
