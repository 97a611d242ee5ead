#!/usr/bin/env python3
"""Headline benchmark: GCN copy_u_sum (g-SpMM) on a 100M-edge RMAT graph.

Metric (BASELINE.json): edges/sec + achieved HBM GB/s, GCN copy_u_sum on a
100M-edge graph, 1/2/4/8 MI355X.

Workload M1: RMAT (a,b,c,d) = (0.57, 0.19, 0.19, 0.05),
scale 23 (N = 8,388,608), E = 100,000,000, vertex ids randomly permuted,
duplicates and self-loops kept, X ~ U(-1, 1) of shape (N, 64) fp32, int32
dst-major CSR.  Generated on the GPU (seeded), CSRs built on the GPU.

A step = one copy_u_sum pass (DGLGraph.update_all(copy_u, sum) lowers to
exactly this call) over the resident graph: out[v] = sum_{u->v} X[u].

Multi-GPU (one process per GPU): `--gpus N` starts the N ranks itself when no
launcher set WORLD_SIZE (launch_ranks), or runs as one rank of a
torch.distributed.run job whose WORLD_SIZE must equal N.  Weak scaling.  The global graph
has N x 100M edges (RMAT scale 23 + log2 N); every rank owns a contiguous
block of destination rows with all their in-edges (1-D row partition, the
halo-subgraph semantics of graph_op.cc:403-509 with num_hops = 1) and holds
the source features replicated (DESIGN.md "Multi-GPU"), so the timed SpMM
has no data-path collective.  `value` = all ranks' edges / max-over-ranks time.

A plain run (`--gpus N --steps K --warmup W`) builds the workload, warms up, times
the K steps and prints the headline line; `--dump-outputs DIR` also writes what the
last timed step computed (dump_outputs).  Everything else -- the workload's
correctness checks, the rocprofv3 PMC passes, the stream-copy probe, update_all,
the CPU baseline, the with-exchange / C4 / C5 lines, the C2 / C3 / C5 configs --
runs only with `--full`.

cpu_baseline (`--full`): the reference's CPU algorithm (out-CSR traversal, OpenMP over
source rows, `omp atomic` scatter; oracle/dgl_ref.c) on a bounded sample of
the same graph, rank 0 at N = 1 only.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(ROOT, "dgl-hack_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch as th  # noqa: E402

RMAT = (0.57, 0.19, 0.19, 0.05)
SCALE = 23
EDGES_PER_GPU = 100_000_000
FEAT = 64
HBM_PEAK_GBPS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec
# xGMI: 7 point-to-point links per GPU at ~153 GB/s each (the task brief's figure; the
# local microarchitecture guide quotes none).  Counted here as ONE direction of one
# link, so the exchange fractions below are, if anything, understated.  In an
# all-to-all over N GPUs of one node a rank uses N - 1 links (one per peer).
XGMI_LINK_GBPS = 153.0


def log(*a):
    if int(os.environ.get("RANK", "0")) == 0:
        print(*a, file=sys.stderr, flush=True)
    trace(*a)


def trace(*a):
    """Per-rank progress file (DGLMI_BENCH_TRACE=dir): where every rank is."""
    d = os.environ.get("DGLMI_BENCH_TRACE")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "rank%s.log" % os.environ.get("RANK", "0")), "a") as fh:
            fh.write("%.2f %s\n" % (time.time(), " ".join(str(x) for x in a)))


def rmat_edges(scale, num_edges, seed, device, chunk=25_000_000):
    """RMAT edge list on the GPU (int32 src, dst), unpermuted ids."""
    a, b, c, _ = RMAT
    gen = th.Generator(device=device)
    gen.manual_seed(seed)
    srcs, dsts = [], []
    done = 0
    while done < num_edges:
        cnt = min(chunk, num_edges - done)
        s = th.zeros(cnt, dtype=th.int32, device=device)
        d = th.zeros(cnt, dtype=th.int32, device=device)
        for lvl in range(scale):
            r = th.rand(cnt, generator=gen, device=device)
            sb = r > (a + b)
            db = ((r > a) & (r <= a + b)) | (r > a + b + c)
            s |= sb.to(th.int32) << lvl
            d |= db.to(th.int32) << lvl
        srcs.append(s)
        dsts.append(d)
        done += cnt
    return th.cat(srcs), th.cat(dsts)


def build_workload(world, rank, device, edges_per_gpu=EDGES_PER_GPU, scale0=SCALE):
    scale = scale0 + int(round(math.log2(world)))
    n = 1 << scale
    m = edges_per_gpu * world
    t0 = time.time()
    src, dst = rmat_edges(scale, m, seed=1234, device=device)
    gp = th.Generator(device=device)
    gp.manual_seed(1)
    perm = th.randperm(n, generator=gp, device=device).to(th.int32)
    src = perm[src.long()]
    dst = perm[dst.long()]
    del perm
    lo = n * rank // world
    hi = n * (rank + 1) // world
    if world > 1:
        keep = (dst >= lo) & (dst < hi)
        src, dst = src[keep], dst[keep] - lo
    gx = th.Generator(device=device)
    gx.manual_seed(2)
    x = th.rand(n, FEAT, generator=gx, device=device) * 2 - 1
    th.cuda.synchronize()
    log("graph generated: scale %d, %d edges total, rank rows [%d, %d), %d local edges (%.1fs)"
        % (scale, m, lo, hi, src.shape[0], time.time() - t0))
    return n, hi - lo, src.contiguous(), dst.contiguous(), x


C4_NODES = 10_000_000
C4_EDGES = 200_000_000


def c4_workload(device, nodes=C4_NODES, edges=C4_EDGES, return_perm=False):
    """Config C4: RMAT scale 24 with ids >= N rejected, N = 10 M,
    E = 200 M, ids permuted (seed 3), X ~ U(-1, 1) of shape (N, 64) (seed 4)."""
    scale = max(1, int(math.ceil(math.log2(nodes))))
    srcs, dsts, have, seed = [], [], 0, 3
    while have < edges:
        want = int((edges - have) * 1.3) + 1024
        s, d = rmat_edges(scale, want, seed=seed * 1000 + len(srcs), device=device)
        ok = (s < nodes) & (d < nodes)
        s, d = s[ok], d[ok]
        take = min(edges - have, int(s.shape[0]))
        srcs.append(s[:take])
        dsts.append(d[:take])
        have += take
    src, dst = th.cat(srcs), th.cat(dsts)
    gp = th.Generator(device=device)
    gp.manual_seed(seed)
    perm = th.randperm(nodes, generator=gp, device=device).to(th.int32)
    src, dst = perm[src.long()], perm[dst.long()]
    if return_perm:  # analysis only (scripts/halo_probe.py): the generator's id map
        return src.contiguous(), dst.contiguous(), perm
    del perm
    gx = th.Generator(device=device)
    gx.manual_seed(4)
    x = th.rand(nodes, FEAT, generator=gx, device=device) * 2 - 1
    return src.contiguous(), dst.contiguous(), x


def measure_c4(world, rank, dist, cdev, device, args):
    """C4 at fixed size (strong scaling): the 10 M-node / 200 M-edge RMAT graph
    split over the ranks by the device label-propagation partitioner
    (``dgl.distributed.partition_labelprop``, standing in for the reference's
    METIS k-way); a step = the halo all-to-all-v of the remote source rows
    (RCCL over xGMI) overlapped with the owned-source half of the aggregation,
    then the halo half (``dgl.distributed.aggregate_with_halo``).  At N = 1 the
    step is one copy_u_sum over the whole graph.  `value` = 200 M edges / step."""
    from dgl import distributed as D
    from dgl import kernel as K
    from dgl.graph_index import device_block_gidx
    t0 = time.time()
    C4_N, C4_E = args.c4_nodes, args.c4_edges
    src, dst, x = c4_workload(device, C4_N, C4_E)
    gidx = device_block_gidx(C4_N, C4_N, src, dst)
    log("C4: graph + CSRs (%.1fs)" % (time.time() - t0))
    out_full = th.empty(C4_N, FEAT, device=device)
    K.copy_reduce("sum", gidx, 0, x, out_full)
    th.cuda.synchronize()
    res = {"workload": "C4: RMAT scale 24 (ids >= 10M rejected), %d nodes, %d edges, feat %d"
                       % (C4_N, C4_E, FEAT), "scaling": "strong", "n_gpus": world,
           "target": "north_star's >= 6x edges/s at 8 GPUs vs 1 is read from this line: a fixed "
                     "graph split over the ranks, the halo exchange inside every step",
           "setup_s": None}
    steps = max(1, args.steps)
    if world > 1:
        # the N = 1 step on the same box in the same run: the whole graph's copy_u_sum
        # on each rank's own GPU (max over ranks) -> speedup_vs_n1
        out1 = th.empty_like(out_full)
        one = lambda: K.copy_reduce("sum", gidx, 0, x, out1)
        for _ in range(2):
            one()
        n1_ms = _max_over_ranks(_timed(one, steps, None, None) * 1e3 / steps, dist, cdev)
        res["n1_ms_per_step"] = n1_ms
        res["n1_edges_per_s"] = C4_E / (n1_ms * 1e-3)
        del out1
    if world == 1:
        out = th.empty_like(out_full)
        step = lambda: K.copy_reduce("sum", gidx, 0, x, out)
        for _ in range(args.warmup):
            step()
        el = _timed(step, steps, None, None)
        if not th.equal(out, out_full):
            raise SystemExit("C4 copy_u_sum not deterministic")
        res.update({"value": C4_E * steps / el, "unit": "edges/s",
                    "ms_per_step": el * 1e3 / steps, "speedup_vs_n1": 1.0, "partitioner": None,
                    "setup_s": time.time() - t0})
        return res
    t1 = time.time()
    assign, info = D.partition_labelprop(gidx, world, rounds=args.c4_rounds, slack=args.c4_slack)
    th.cuda.synchronize()
    lp_s = time.time() - t1
    # every rank computed the same labels (deterministic kernels); make sure of it
    if not _ranks_agree(assign, dist, cdev):
        raise SystemExit("ranks disagree on the partition")
    trace("C4: hash check done")
    log("C4: label propagation %.2fs" % lp_s)
    trace("C4: hash check")
    stats_lp = D.partition_stats(src, dst, assign, world)
    contig = D.contiguous_parts_device((gidx.in_csr.degrees() + 1).to(th.int32), world)
    stats_ct = D.partition_stats(src, dst, contig, world)
    del contig
    log("C4: partition stats (%.1fs)" % (time.time() - t0))
    part = D.build_partition_from_assignment(src, dst, assign, rank, None, world,
                                             exchange="hybrid", tau=args.c4_tau)
    log("C4: hybrid plan (%.1fs)" % (time.time() - t0))
    pull = D.build_partition_from_assignment(src, dst, assign, rank, None, world)
    pull.release_edges()
    pull.split_gidx()
    del gidx, src, dst
    x_inner = x[part.inner_global].contiguous()
    ref = out_full[part.inner_global]
    del out_full, x
    th.cuda.synchronize()
    f = FEAT
    bufs = D.hybrid_buffers(x_inner, part)
    out = th.empty(part.n_inner, f, device=device)
    step = lambda: D.aggregate_hybrid(x_inner, part, out, None, bufs)
    send_p = th.empty(int(pull.send_counts.sum()), f, device=device)
    recv_p = th.empty(pull.n_halo, f, device=device)
    tmp_p = th.empty(pull.n_inner, f, device=device)
    out_p = th.empty(pull.n_inner, f, device=device)
    pstep = lambda: D.aggregate_with_halo(x_inner, pull, out_p, None, recv_p, send_p, tmp_p)
    log("C4: pull plan (%.1fs)" % (time.time() - t0))
    step()
    pstep()
    th.cuda.synchronize()
    log("C4: first steps (%.1fs)" % (time.time() - t0))
    scale = ref.abs().max().clamp(min=1e-30)
    err = _max_over_ranks(float((out - ref).abs().max() / scale), dist, cdev)
    perr = _max_over_ranks(float((out_p - ref).abs().max() / scale), dist, cdev)
    if max(err, perr) > 1e-4:
        raise SystemExit("C4 partitioned copy_u_sum differs from the single-GPU one: "
                         "hybrid %g, pull %g" % (err, perr))
    for _ in range(args.warmup):
        step()
        pstep()
    el = _timed(step, steps, dist, cdev)
    pel = _timed(pstep, steps, dist, cdev)
    rc, sc = pull.recv_counts.tolist(), pull.send_counts.tolist()
    ex = _timed(lambda: D._a2av(recv_p, th.index_select(x_inner, 0, pull.send_idx, out=send_p),
                                rc, sc, None), steps, dist, cdev)
    moved = th.tensor([float(part.rows_moved()), float(pull.n_halo)], device=cdev,
                      dtype=th.float64)
    dist.all_reduce(moved)
    # per-rank SpMM work of the hybrid step (edges walked: owned block + push block +
    # receive block) -- the push side moves work to the hub sources' owners
    nnz = lambda gi: gi.in_csr.nnz if gi is not None else 0
    work = th.tensor([float(nnz(part.g_own) + nnz(part.g_push) + nnz(part.g_recv))],
                     device=cdev, dtype=th.float64)
    works = [th.zeros_like(work) for _ in range(world)]
    dist.all_gather(works, work)
    works = [int(w.item()) for w in works]
    per_rank, ex_sum, model = c4_decomposition(part, x_inner, bufs, out, steps, rank, world,
                                               dist, cdev)
    res.update({"value": C4_E * steps / el, "unit": "edges/s", "ms_per_step": el * 1e3 / steps,
                "per_rank": per_rank, "exchange_aggregate": ex_sum, "model": model,
                "speedup_vs_n1": res["n1_ms_per_step"] / (el * 1e3 / steps),
                "exchange": "hybrid: pulled rows + pushed partial sums (tau %d), two "
                            "all-to-all-v (%s) overlapped with the owned-source SpMM"
                            % (args.c4_tau, dist.get_backend()),
                "rows_moved_per_step": int(moved[0].item()),
                "spmm_edges_per_rank": works,
                "bytes_moved_per_step": int(moved[0].item()) * 4 * f,
                "pull_only": {"ms_per_step": pel * 1e3 / steps,
                              "edges_per_s": C4_E * steps / pel,
                              "rows_moved_per_step": int(moved[1].item()),
                              "exchange_only_ms": ex * 1e3 / steps},
                "partitioner": "device label propagation, %d rounds, edge-balanced, slack %g "
                               "(%.2fs)" % (args.c4_rounds, args.c4_slack, lp_s),
                "rel_err_vs_single_gpu": max(err, perr),
                "halo_rows_pull": stats_lp["halo_rows"], "edges_per_part": stats_lp["edges"],
                "cut_fraction": stats_lp["cut_edges"] / C4_E,
                "contiguous_partition": {"halo_rows_pull": stats_ct["halo_rows"],
                                         "edges_per_part": stats_ct["edges"],
                                         "cut_fraction": stats_ct["cut_edges"] / C4_E},
                "setup_s": time.time() - t0})
    return res


def c4_decomposition(part, x_inner, bufs, out, steps, rank, world, dist, cdev):
    """The hybrid C4 step taken apart on every rank (round 5): each block's copy_u_sum
    alone (owned, push, receive) with its algorithmic bytes and HBM fraction, the two
    all-to-all-v alone (pulled rows, then partial rows; send buffers filled once) with
    the bytes this rank sends and receives and their rate against the xGMI links, and
    the step the schedule predicts from those parts -- the exchange in flight from the
    start, the push and owned SpMMs meanwhile, the receive pass after both:
    max(t_push + t_own, t_exchange) + t_recv, max over ranks -- to set beside the
    measured step."""
    from dgl import distributed as D
    from dgl import kernel as K
    f = FEAT
    send, recv, pout, tmp = bufs["send"], bufs["recv"], bufs["pout"], bufs["tmp"]
    th.index_select(x_inner, 0, part.send_idx, out=send)
    blocks = (("own", part.g_own, x_inner, tmp, None),
              ("push", part.g_push, x_inner, pout, None),
              ("recv", part.g_recv, recv, out, (None, None, None, tmp)))
    spmm = {}
    for name, gi, src, dst, epi in blocks:
        if gi is None:
            spmm[name] = {"edges": 0, "alg_bytes": 0, "ms": 0.0, "GBps": None, "frac": None}
            continue
        fn = (lambda gi=gi, src=src, dst=dst, epi=epi:
              K.copy_reduce("sum", gi, 0, src, dst, epilogue=epi))
        fn()
        t = _timed(fn, steps, None, None) * 1e3 / steps
        b = spmm_alg_bytes(gi, f, addend=epi is not None)
        spmm[name] = {"edges": int(gi.in_csr.nnz), "alg_bytes": b, "ms": t,
                      "GBps": b / (t * 1e-3) / 1e9, "frac": b / (t * 1e-3) / 1e9 / HBM_PEAK_GBPS}
    if part.g_push is not None:  # the partial rows the peers will receive
        K.copy_reduce("sum", part.g_push, 0, x_inner, pout)
    rc, sc = part.recv_counts.tolist(), part.send_counts.tolist()
    pc, oc = part.pin_counts.tolist(), part.pout_counts.tolist()

    def exchange():
        D._a2av(recv[:part.n_halo], send, rc, sc, None)
        D._a2av(recv[part.n_halo:], pout, pc, oc, None)
    exchange()
    ex_mine, _ = _timed_local(exchange, steps, dist, cdev)
    ex_ms = ex_mine * 1e3 / steps
    sent = int(part.send_counts.sum()) + int(part.pout_counts.sum())
    got = int(part.n_halo) + int(part.n_pin)
    sp_bytes = sum(v["alg_bytes"] for v in spmm.values())
    sp_ms = sum(v["ms"] for v in spmm.values())
    rec = {"rank": rank, "spmm_edges": sum(v["edges"] for v in spmm.values()),
           "spmm_alg_bytes": sp_bytes, "spmm_ms": sp_ms,
           "spmm_GBps": sp_bytes / (sp_ms * 1e-3) / 1e9 if sp_ms > 0 else None,
           "spmm_frac": sp_bytes / (sp_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS if sp_ms > 0 else None,
           "blocks": spmm, "rows_sent": sent, "rows_received": got,
           "bytes_sent": sent * 4 * f, "bytes_received": got * 4 * f, "exchange_ms": ex_ms,
           "model_ms": max(spmm["push"]["ms"] + spmm["own"]["ms"], ex_ms) + spmm["recv"]["ms"]}
    per_rank = gather_ranks(rec, dist)
    ex_sum = exchange_summary(per_rank, world)
    tot_b = sum(r["spmm_alg_bytes"] for r in per_rank)
    t_max = max(r["spmm_ms"] for r in per_rank)
    model = {"step_ms": max(r["model_ms"] for r in per_rank),
             "rule": "max over ranks of max(t_push + t_own, t_exchange) + t_recv, each part "
                     "timed alone on the rank (owned SpMM and exchange overlap; push before, "
                     "receive pass after)",
             "spmm_aggregate": {"alg_bytes": tot_b, "max_rank_ms": t_max,
                                "GBps": tot_b / (t_max * 1e-3) / 1e9 if t_max > 0 else None,
                                "frac": (tot_b / (t_max * 1e-3) / 1e9 / (world * HBM_PEAK_GBPS)
                                         if t_max > 0 else None),
                                "peak_GBps": world * HBM_PEAK_GBPS}}
    return per_rank, ex_sum, model


C5_NODES = 5_000_000
C5_EDGES = 80_000_000
C5_RELS = 4


def _allreduce_sum(tensors, dist, cdev):
    """Sum of the tensors over the ranks, in place (one flat collective; host
    staging for gloo)."""
    flat = th.cat([t.reshape(-1) for t in tensors])
    if cdev == "cpu":
        f = flat.cpu()
        dist.all_reduce(f)
        flat.copy_(f)
    else:
        dist.all_reduce(flat)
    off = 0
    for t in tensors:
        t.copy_(flat[off:off + t.numel()].view_as(t))
        off += t.numel()


def measure_c5(world, rank, dist, cdev, device, args):
    """C5 at N > 1 (BASELINE.json config 5: R-GCN on a 4-relation 5 M-node / 80 M-edge
    graph on 4 MI355X): DistRelGraphConv (64 -> 64, basis, self-loop, bias, norm = 1 /
    in-degree) on each rank's block of the device label-propagation partition
    (METIS stand-in), the fused R-GCN kernels on the local block.  A step = forward
    (halo all-to-all-v of the remote input rows) + backward (the reverse exchange of
    the halo rows' gradients) + the weight-gradient all-reduce -- the reference's
    multi-GPU pattern (examples/pytorch/graphsage/train_sampling_multi_gpu.py:193-265)
    on a full-graph partition.  Before timing, every rank runs the single-GPU module
    on the whole graph and the partitioned outputs, input gradients and all-reduced
    weight gradients must match it; that whole-graph step, timed on each rank's own
    GPU, is the N = 1 figure of speedup_vs_n1.  Strong scaling: value = 80 M edges /
    step time."""
    from dgl import distributed as D
    from dgl.nn.pytorch import RelGraphConv
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import bench_configs as bc
    t0 = time.time()
    n, m, R, f = args.c5_nodes, args.c5_edges, C5_RELS, FEAT
    g = bc.chung_lu(n, m, 0.5, 8, device)  # the graph of the N = 1 configs line
    src, dst = g._graph._device_only
    gen = th.Generator(device=device)
    gen.manual_seed(8)
    et = th.randint(0, R, (m,), generator=gen, device=device)
    if not (_ranks_agree(src, dist, cdev) and _ranks_agree(dst, dist, cdev)
            and _ranks_agree(et, dist, cdev)):
        raise SystemExit("C5: ranks built different graphs")
    indeg = th.bincount(dst.long(), minlength=n).float().clamp(min=1)
    norm = (1.0 / indeg)[dst.long()].reshape(m, 1)
    del indeg
    gen.manual_seed(9)
    x = th.randn(n, f, generator=gen, device=device)
    go = th.randn(n, f, generator=gen, device=device)
    th.manual_seed(0)
    conv = RelGraphConv(f, f, R, "basis", num_bases=R, self_loop=True).to(device)
    with th.no_grad():
        conv.h_bias.uniform_(-0.5, 0.5)
    params = list(conv.parameters())
    xr = x.clone().requires_grad_()
    out_full = conv(g, xr, et, norm)
    grads_full = th.autograd.grad(out_full, [xr] + params, go)
    out_full = out_full.detach()

    def step1():
        th.autograd.grad(conv(g, xr, et, norm), [xr] + params, go)
    steps = max(1, min(args.steps, 10))
    for _ in range(2):
        step1()
    n1_ms = _max_over_ranks(_timed(step1, steps, None, None) * 1e3 / steps, dist, cdev)
    del xr
    log("C5: whole-graph module + N = 1 timing (%.1fs)" % (time.time() - t0))
    gidx = g._graph.get_immutable_gidx(device)
    t1 = time.time()
    assign, info = D.partition_labelprop(gidx, world, rounds=args.c4_rounds, slack=args.c4_slack)
    th.cuda.synchronize()
    lp_s = time.time() - t1
    if not _ranks_agree(assign, dist, cdev):
        raise SystemExit("C5: ranks disagree on the partition")
    part = D.build_partition_from_assignment(src, dst, assign, rank, None, world)
    keep = assign[dst.long()] == rank  # local edge order = the global order of kept edges
    et_l, norm_l = et[keep].contiguous(), norm[keep].contiguous()
    del keep, src, dst, assign
    g._graph.__dict__.pop("_rgcn_fused", None)  # the whole graph's prepared state
    gidx.__dict__.pop("_rgcn_state", None)
    log("C5: partition (%.1fs)" % (time.time() - t0))
    dr = D.DistRelGraphConv(f, f, R, "basis", num_bases=R, self_loop=True).to(device)
    dr.conv.load_state_dict(conv.state_dict())
    inner = part.inner_global.long()
    xi = x[inner].contiguous().requires_grad_()
    go_i = go[inner].contiguous()
    params_d = list(dr.parameters())
    out_d = dr(part, xi, et_l, norm_l)
    fused = part.local_graph(device)._graph.__dict__.get("_rgcn_fused") is not None
    grads_d = list(th.autograd.grad(out_d, [xi] + params_d, go_i))
    _allreduce_sum(grads_d[1:], dist, cdev)
    ref = out_full[inner]
    out_err = float(((out_d.detach() - ref).abs() / (1e-4 + 1e-4 * ref.abs())).max())
    gx_ref = grads_full[0][inner]
    errs = [float((grads_d[0] - gx_ref).abs().max()) / (1e-3 + 1e-4 * float(gx_ref.abs().max()))]
    for a, b in zip(grads_d[1:], grads_full[1:]):
        errs.append(float((a - b).abs().max()) / (1e-3 + 1e-4 * float(b.abs().max())))
    worst = _max_over_ranks(max([out_err] + errs), dist, cdev)
    all_fused = _max_over_ranks(0.0 if fused else 1.0, dist, cdev) == 0.0
    if worst > 1.0:
        raise SystemExit("C5: the partitioned R-GCN layer differs from the single-GPU module "
                         "(worst error / bound %.3g)" % worst)
    del out_d, grads_d, out_full, grads_full, ref, gx_ref, g, gidx, x, go
    th.cuda.empty_cache()

    def dstep():
        for p in params_d:
            p.grad = None
        xi.grad = None
        dr(part, xi, et_l, norm_l).backward(go_i)
        D.allreduce_gradients(params_d, average=False)

    def fstep():
        with th.no_grad():
            dr(part, xi, et_l, norm_l)
    for _ in range(2):
        dstep()
        fstep()
    el = _timed(dstep, steps, dist, cdev)
    fel = _timed(fstep, steps, dist, cdev)
    halo = th.tensor([float(part.n_halo)], device=cdev, dtype=th.float64)
    dist.all_reduce(halo)
    ms = el * 1e3 / steps
    # the step taken apart on every rank (round 5): the layer's forward + backward on
    # the local block with the halo rows already in place, and the two exchanges alone
    # (the forward's all-to-all-v of halo input rows, the backward's reverse one)
    g_loc = part.local_graph(device)
    x_full = D.halo_exchange(xi.detach(), part).detach().requires_grad_()
    n_in = part.n_inner

    def cstep():
        th.autograd.grad(dr.conv(g_loc, x_full, et_l, norm_l)[:n_in], [x_full] + params_d, go_i)
    cstep()
    c_ms = _timed(cstep, steps, None, None) * 1e3 / steps
    idx = part.device_plan(xi.device)
    send = xi.detach().index_select(0, idx).contiguous()
    recv = xi.new_empty((part.n_halo, f))
    rc, sc = part.recv_counts.tolist(), part.send_counts.tolist()

    def xstep():
        D._a2av(recv, send, rc, sc, None)   # forward: halo input rows in
        D._a2av(send, recv, sc, rc, None)   # backward: their gradients back out
    xstep()
    x_mine, _ = _timed_local(xstep, steps, dist, cdev)
    x_ms = x_mine * 1e3 / steps
    e_loc = int(g_loc.number_of_edges())
    rows = int(part.n_halo) + int(sum(sc))
    # bytes model of the fused R-GCN walks: one gathered 4F-byte row per edge each way
    # (forward: the relation-transformed source row; backward: the gradient row) plus
    # 12 B of column id, edge type and norm per edge each way
    b_model = 2 * e_loc * (4 * f + 12)
    rec = {"rank": rank, "local_edges": e_loc, "halo_rows": int(part.n_halo),
           "compute_ms": c_ms, "compute_edges_per_s": e_loc / (c_ms * 1e-3),
           "compute_alg_bytes": b_model,
           "compute_GBps": b_model / (c_ms * 1e-3) / 1e9,
           "compute_frac": b_model / (c_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS,
           "rows_exchanged": rows,
           # forward: n_halo rows in, sum(sc) out; backward: the reverse
           "bytes_received": rows * 4 * f, "bytes_sent": rows * 4 * f,
           "exchange_ms": x_ms}
    per_rank = gather_ranks(rec, dist)
    ex_sum = exchange_summary(per_rank, world)
    n1_rate = m / (n1_ms * 1e-3)
    for r in per_rank:
        r["compute_rate_vs_n1"] = r["compute_edges_per_s"] / n1_rate
    del x_full, send, recv
    return {"workload": "C5: R-GCN RelGraphConv 4 relations basis 64->64, self-loop + bias, "
                        "norm 1/in-degree, Chung-Lu(0.5) %d nodes / %d typed edges" % (n, m),
            "scaling": "strong", "n_gpus": world, "value": m * steps / el, "unit": "edges/s",
            "ms_per_step": ms, "fwd_ms": fel * 1e3 / steps,
            "step": "DistRelGraphConv forward (halo all-to-all-v) + backward (reverse halo "
                    "exchange) + weight-gradient all-reduce (%s)" % dist.get_backend(),
            "n1_ms_per_step": n1_ms, "n1_step": "RelGraphConv forward + backward on the whole "
                                                "graph, each rank's own GPU, max over ranks",
            "speedup_vs_n1": n1_ms / ms, "fused_route_all_ranks": all_fused,
            "check_worst_err_over_bound": worst,
            "check": "partitioned output (rtol = atol = 1e-4), input gradient and all-reduced "
                     "weight gradients (1e-3 + 1e-4 max|ref|) vs the whole-graph module",
            "partitioner": "device label propagation, %d rounds, slack %g (%.2fs)"
                           % (args.c4_rounds, args.c4_slack, lp_s),
            "halo_rows_all_ranks": int(halo.item()), "per_rank": per_rank,
            "exchange_aggregate": ex_sum,
            "model": {"step_ms": max(r["compute_ms"] + r["exchange_ms"] for r in per_rank),
                      "rule": "max over ranks of compute (local block, halo rows in place) + "
                              "exchange (forward rows in, backward gradients out), each timed "
                              "alone: the layer's exchanges are not overlapped"},
            "setup_s": time.time() - t0}


def make_local_graph(n_src, n_dst, src, dst, device):
    """Local in-CSR (rows = owned dst, cols = global src) built on the GPU."""
    from dgl.graph_index import device_block_gidx
    g = device_block_gidx(n_src, n_dst, src, dst)
    return g, (g.out_csr.indptr, g.out_csr.indices)


def _physical_cores():
    """Physical cores of the host (distinct (package, core id) pairs)."""
    seen, phys, core = set(), None, None
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("physical id"):
                phys = line.split(":", 1)[1].strip()
            elif line.startswith("core id"):
                core = line.split(":", 1)[1].strip()
            elif not line.strip() and core is not None:
                seen.add((phys, core))
                phys = core = None
    except OSError:
        return None
    return len(seen) or None


def cpu_baseline(o_ptr, o_idx, x, n_dst, sample_edges=40_000_000, warmup=3, reps=10):
    """The reference's CPU algorithm (out-CSR traversal, OpenMP over source rows,
    `omp atomic` scatter, zero fill of every destination row) on the leading
    source rows of the M1 out-CSR holding `sample_edges` edges (a bounded sample:
    ~1-2 s per pass on the box's 16-CPU lease), median of `reps` passes after
    `warmup` passes."""
    from oracle import oracle as O
    affinity = len(os.sched_getaffinity(0))
    phys = _physical_cores()
    env_threads = int(os.environ.get("OMP_NUM_THREADS", "0") or 0)
    # the lease's CPU share: OMP_NUM_THREADS as the harness sets it (16 per GPU on
    # the MI355X boxes), else every CPU this process may run on, never more than
    # the physical cores
    threads = env_threads or affinity
    if phys:
        threads = min(threads, phys)
    threads = max(1, min(threads, O.max_threads() if not env_threads else threads))
    ptr = o_ptr.cpu().numpy()
    rows = ptr.shape[0] - 1
    if sample_edges is not None:
        rows = max(1, min(rows, int(np.searchsorted(ptr, sample_edges, side="right")) - 1))
    e = int(ptr[rows])
    idx = o_idx[:e].cpu().numpy().astype(np.int32)
    xs = np.ascontiguousarray(x[:rows].cpu().numpy())  # features of the sampled source rows
    ptr_s = ptr[:rows + 1].astype(np.int32)
    for _ in range(warmup):
        O.copy_src_sum_i32(rows, ptr_s, idx, xs, n_dst, threads)
    times = []
    for _ in range(reps):
        t0 = time.time()
        O.copy_src_sum_i32(rows, ptr_s, idx, xs, n_dst, threads)
        times.append(time.time() - t0)
    t = float(np.median(times))
    model = None
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return {"value": e / t, "unit": "edges/s", "cores": threads, "kind": "port",
            "cpu_model": model, "host_cpus": os.cpu_count(), "affinity_cpus": affinity,
            "physical_cores": phys, "omp_num_threads_env": env_threads or None,
            "sample": "reference CPU algorithm (oracle/dgl_ref.c ref_copy_src_sum_i32: out-CSR, "
                      "OpenMP over src rows, omp-atomic scatter, zero fill of all %d dst rows) on "
                      "the first %d source rows (%d edges) of the M1 out-CSR, F=%d, median of %d "
                      "passes after %d warm-up passes, %d OpenMP threads (the lease's CPU share: "
                      "OMP_NUM_THREADS as set by the harness, capped by affinity and physical cores)"
                      % (n_dst, rows, e, FEAT, reps, warmup, threads),
            "seconds_per_pass": t}


PMC_PASSES = (("FETCH_SIZE",), ("WRITE_SIZE",), ("TCC_HIT_sum", "TCC_MISS_sum"))


def _rocprof():
    import shutil
    return shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3"
                                         if os.path.exists("/opt/rocm/bin/rocprofv3") else None)


def pmc_child(world=1, rank=0, edges_per_gpu=EDGES_PER_GPU, scale0=SCALE):
    """Body of one rocprofv3 --pmc pass (``bench.py --pmc-child``): this rank's M1
    launch pair (its row block of the world-size graph, as the timed run builds it)
    3 times, then 3 launches over a calibration graph whose bytes are known exactly
    (a random permutation of the same node table: every source row gathered once, no
    reuse).  The parent makes the rank's GPU the only visible one (cuda:0 here)."""
    import dgl  # noqa: F401
    from dgl import kernel as K
    from dgl.graph_index import device_block_gidx
    device = "cuda:0"
    th.cuda.set_device(0)
    n, n_dst, src, dst, x = build_workload(world, rank, device, edges_per_gpu, scale0)
    g, _ = make_local_graph(n, n_dst, src, dst, device)
    del src, dst
    out = th.empty(n_dst, FEAT, device=device)
    for _ in range(3):
        K.copy_reduce("sum", g, 0, x, out)
    th.cuda.synchronize()
    del g, out
    gp = th.Generator(device=device)
    gp.manual_seed(11)
    csrc = th.randperm(n, generator=gp, device=device).to(th.int32)
    cdst = th.arange(n, dtype=th.int32, device=device)
    gc = device_block_gidx(n, n, csrc, cdst)
    out = th.empty(n, FEAT, device=device)
    for _ in range(3):
        K.copy_reduce("sum", gc, 0, x, out)
    th.cuda.synchronize()


def pmc_phase_values(rows, n_passes, launches=3):
    """Counter values of the PMC child's launches by phase.  rows: (pass, dispatch id,
    is_reduce, counter, value) of the k_chunk_reduce / k_chunk_fixup dispatches.
    Within each pass, dispatch order tells the phases apart: the first `launches`
    reduce launches and the fixups after them are the rank's M1 launches ("m1"), the
    rest the calibration graph's ("cal").  Returns {(phase, counter): [values]}."""
    vals = {}
    for i in range(n_passes):
        disp = sorted({(d, red) for pi, d, red, _, _ in rows if pi == i})
        phase, nred, phase_of = "m1", 0, {}
        for d, red in disp:
            if red:
                nred += 1
                phase = "m1" if nred <= launches else "cal"
            phase_of[d] = phase
        for pi, d, red, cname, v in rows:
            if pi == i:
                vals.setdefault((phase_of[d], cname), []).append(v)
    return vals


def _child_device_env(local):
    """Environment that leaves a child process exactly one GPU: this rank's.  The
    rank's device is the `local`-th one this process would see (ROCR_VISIBLE_DEVICES
    and then HIP_/CUDA_VISIBLE_DEVICES filter it), pinned through ROCR_VISIBLE_DEVICES
    so the profiler's agent list holds that GPU alone."""
    env = dict(os.environ)
    idx = str(local)
    for var in ("CUDA_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES"):
        lst = env.pop(var, None)
        if lst:
            idx = lst.split(",")[int(idx)]
    rocr = env.get("ROCR_VISIBLE_DEVICES")
    env["ROCR_VISIBLE_DEVICES"] = rocr.split(",")[int(idx)] if rocr else idx
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR",
              "MASTER_PORT", "GROUP_RANK", "ROLE_RANK"):
        env.pop(k, None)
    return env


def pmc_traffic_live(world=1, rank=0, local=0, edges_per_gpu=EDGES_PER_GPU, scale0=SCALE,
                     timeout_s=240):
    """Fabric bytes of this rank's copy_u_sum launch pair, measured now by rocprofv3
    PMC passes over ``bench.py --pmc-child`` (one counter group per pass, as
    MI355X_MICROARCH.md §rocprofv3 prescribes) on this rank's own GPU, run BEFORE
    this process touches the GPU.  gfx950 FETCH_SIZE under-reports wide reads
    (MI355X_MICROARCH.md §HBM), so its scale is calibrated in the same pass on a
    permutation gather whose read bytes are known exactly (4F per source row + 8 per
    edge); WRITE_SIZE is exact for 16-B stores.  Ranks sharing one GPU (a
    --same-device rehearsal) take turns through a lock file.  Returns a dict or None."""
    import csv
    import fcntl
    import glob
    import shutil
    import signal
    import subprocess
    import tempfile
    prof = _rocprof()
    if prof is None:
        return None
    env = _child_device_env(local)
    tmp = tempfile.mkdtemp(prefix="dglmi_pmc_")
    lock = open(os.path.join(tempfile.gettempdir(), "dglmi_pmc_gpu%s.lock"
                             % env["ROCR_VISIBLE_DEVICES"]), "w")
    fcntl.flock(lock, fcntl.LOCK_EX)
    rows = []
    try:
        for i, counters in enumerate(PMC_PASSES):
            d = os.path.join(tmp, "p%d" % i)
            cmd = [prof, "--pmc", *counters, "-d", d, "-o", "run", "--output-format", "csv", "--",
                   sys.executable, os.path.abspath(__file__), "--pmc-child",
                   "--pmc-world", str(world), "--pmc-rank", str(rank),
                   "--edges-per-gpu", str(edges_per_gpu), "--scale", str(scale0)]
            p = subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                                 start_new_session=True, cwd=ROOT, env=env)
            try:
                _, err = p.communicate(timeout=timeout_s)
            except subprocess.TimeoutExpired:
                os.killpg(p.pid, signal.SIGKILL)
                p.wait()
                log("pmc pass %s timed out" % (counters,))
                return None
            if p.returncode != 0:
                log("pmc pass %s failed rc=%d: %s" % (counters, p.returncode,
                                                      err.decode(errors="replace")[-500:]))
                return None
            files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
            if not files:
                return None
            for r in csv.DictReader(open(files[0])):
                name = r["Kernel_Name"]
                if "k_chunk_reduce" in name or "k_chunk_fixup" in name:
                    rows.append((i, int(r["Dispatch_Id"]), "k_chunk_reduce" in name,
                                 r["Counter_Name"], float(r["Counter_Value"])))
    finally:
        fcntl.flock(lock, fcntl.LOCK_UN)
        lock.close()
        shutil.rmtree(tmp, ignore_errors=True)
    vals = pmc_phase_values(rows, len(PMC_PASSES))

    def per_launch(phase, counter):  # mean per launch pair (reduce + fixup sums / 3)
        v = vals.get((phase, counter))
        return float(np.sum(v)) / 3.0 if v else 0.0

    n = 1 << (scale0 + int(round(math.log2(world))))
    cal_known_read = 4 * FEAT * n + 8 * n  # every X row once + rows/indices stream
    fetch_cal = per_launch("cal", "FETCH_SIZE") * 1024
    fetch = per_launch("m1", "FETCH_SIZE") * 1024
    write = per_launch("m1", "WRITE_SIZE") * 1024
    if fetch_cal <= 0 or fetch <= 0:
        return None
    scale = cal_known_read / fetch_cal
    hit = per_launch("m1", "TCC_HIT_sum")
    miss = per_launch("m1", "TCC_MISS_sum")
    return {"bytes_per_launch": scale * fetch + write, "read_bytes": scale * fetch,
            "write_bytes": write, "fetch_size_bytes_raw": fetch, "fetch_scale": scale,
            "fetch_scale_from": "permutation gather, %d known read bytes, FETCH_SIZE %d"
                                % (cal_known_read, fetch_cal),
            "l2_hit_rate": hit / (hit + miss) if hit + miss > 0 else None,
            "passes": [list(c) for c in PMC_PASSES], "rank": rank,
            "device": "ROCR_VISIBLE_DEVICES=%s" % env["ROCR_VISIBLE_DEVICES"],
            "method": "rocprofv3 --pmc per pass over `bench.py --pmc-child` (this rank's launch "
                      "pair x3 on its own GPU), read = FETCH_SIZE x calibrated scale, + "
                      "WRITE_SIZE; Infinity-Cache hits included (they leave L2)"}


def _max_over_ranks(v, dist, cdev):
    """max of a float over all ranks (so every rank takes the same exit path)."""
    if dist is None:
        return float(v)
    t = th.tensor([float(v)], device=cdev, dtype=th.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def _ranks_agree(t, dist, cdev):
    """True when an integer device tensor is the same on every rank (a position-weighted
    checksum mod a prime, compared by max and min over the ranks)."""
    h = (t.reshape(-1).long() * th.arange(1, t.numel() + 1, device=t.device) % 1000003).sum()
    hs = th.tensor([float(h.item())], device=cdev, dtype=th.float64)
    hmax, hmin = hs.clone(), hs.clone()
    dist.all_reduce(hmax, op=dist.ReduceOp.MAX)
    dist.all_reduce(hmin, op=dist.ReduceOp.MIN)
    return float(hmax.item()) == float(hmin.item())


def _timed(fn, steps, dist, cdev):
    """barrier + sync bracketed wall time of `steps` calls, max over ranks (s)."""
    if dist is not None:
        dist.barrier()
    th.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    th.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    el = time.perf_counter() - t
    if dist is not None:
        v = th.tensor([el], device=cdev, dtype=th.float64)
        dist.all_reduce(v, op=dist.ReduceOp.MAX)
        el = float(v.item())
    return el


def _timed_local(fn, steps, dist, cdev):
    """As _timed, but returns (this rank's own seconds, max over ranks)."""
    if dist is not None:
        dist.barrier()
    th.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    th.cuda.synchronize()
    mine = time.perf_counter() - t
    if dist is not None:
        dist.barrier()
    return mine, _max_over_ranks(mine, dist, cdev)


def spmm_alg_bytes(gi, feat, addend=False):
    """SURVEY §8(d)'s algorithmic bytes of one copy_u_sum over block ``gi``: indptr +
    column ids + one gathered 4F-byte source row per edge + one 4F-byte output row per
    destination (+ the epilogue's addend row)."""
    if gi is None:
        return 0
    c = gi.in_csr
    rows, nnz = int(c.num_rows), int(c.nnz)
    return 4 * (rows + 1) + 4 * nnz + 4 * feat * nnz + 4 * feat * rows * (2 if addend else 1)


def gather_ranks(rec, dist):
    """Every rank's record (a dict) on every rank, in rank order."""
    if dist is None:
        return [rec]
    out = [None] * dist.get_world_size()
    dist.all_gather_object(out, rec)
    return out


def exchange_summary(per_rank, world, bytes_key_in="bytes_received", bytes_key_out="bytes_sent",
                     ms_key="exchange_ms"):
    """Per-rank achieved exchange rates against the xGMI links a rank uses in an
    all-to-all (N - 1, one per peer) and the job's aggregate: the bytes that crossed
    the fabric (each row counted once, at its receiver) over the slowest rank's
    exchange time, against N (N - 1) links.  Adds fields to ``per_rank`` in place."""
    links = max(world - 1, 1)
    for r in per_rank:
        t = r.get(ms_key) or 0.0
        r["exchange_in_GBps"] = r[bytes_key_in] / (t * 1e-3) / 1e9 if t > 0 else None
        r["exchange_out_GBps"] = r[bytes_key_out] / (t * 1e-3) / 1e9 if t > 0 else None
        r["xgmi_peak_GBps"] = links * XGMI_LINK_GBPS
        busy = max(r["exchange_in_GBps"] or 0.0, r["exchange_out_GBps"] or 0.0)
        r["exchange_frac"] = busy / r["xgmi_peak_GBps"] if t > 0 else None
    tmax = max((r.get(ms_key) or 0.0) for r in per_rank)
    total = sum(r[bytes_key_in] for r in per_rank)
    agg = total / (tmax * 1e-3) / 1e9 if tmax > 0 else None
    peak = world * links * XGMI_LINK_GBPS
    return {"bytes_all_ranks": total, "max_exchange_ms": tmax, "GBps": agg, "peak_GBps": peak,
            "frac": agg / peak if agg else None,
            "peak_note": "N (N - 1) x %g GB/s: every rank on its N - 1 peer links, one "
                         "direction each (task brief's per-link figure)" % XGMI_LINK_GBPS}


# Exit status of a run whose headline line was printed but one of its side lines
# (with-exchange, C4) failed: the line carries the errors under
# `side_line_errors`, and the status tells the caller without parsing it.
SIDE_LINE_RC = 3


class SideLineGuard:
    """N > 1 only.  The side lines after the headline (with-exchange, C4) run
    collectives.  If one rank raises or stalls there, its peers wait inside RCCL,
    and the launcher would end the job without the headline line.  So a failing
    rank posts its error in the job's TCP store; rank 0's watchdog thread then
    prints the line with the error recorded under the phase that failed (and in
    `side_line_errors`), and every rank leaves with status SIDE_LINE_RC.  A phase
    that exceeds `budget_s` counts as failed."""

    KEY_ERR = "dglmi_bench_side_error"
    KEY_DONE = "dglmi_bench_line_printed"

    def __init__(self, dist, rank, res, budget_s=300.0, poll_s=0.25):
        import threading
        self.store = dist.distributed_c10d._get_default_store()
        self.rank, self.res, self.budget_s, self.poll_s = rank, res, budget_s, poll_s
        self.phase = None
        self.t_phase = time.time()
        self.lock = threading.Lock()
        self.printed = False
        self.thread = threading.Thread(target=self._watch, daemon=True)
        self.thread.start()

    def start(self, phase):
        self.phase, self.t_phase = phase, time.time()

    def _emit_and_exit(self, err):
        with self.lock:
            if not self.printed:
                self.printed = True
                phase = self.phase or "side_line"
                self.res[phase] = {"error": err}
                self.res.setdefault("side_line_errors", []).append({"line": phase, "error": err})
                print(json.dumps(self.res), flush=True)
            try:
                self.store.set(self.KEY_DONE, "1")
            except Exception:  # noqa: BLE001
                pass
            os._exit(SIDE_LINE_RC)

    def _watch(self):
        seen = None
        while True:
            time.sleep(self.poll_s)
            if self.printed:
                return
            try:
                if (self.rank == 0 and self.phase is not None
                        and time.time() - self.t_phase > self.budget_s):
                    self.store.set(self.KEY_ERR, "%s exceeded %.0f s" % (self.phase, self.budget_s))
                if seen is None and self.store.check([self.KEY_ERR]):
                    seen = time.time()
                if seen is not None and self.rank == 0:
                    self._emit_and_exit(self.store.get(self.KEY_ERR).decode())
                if seen is not None and self.store.check([self.KEY_DONE]):
                    os._exit(SIDE_LINE_RC)
            except Exception:  # noqa: BLE001  (store gone: rank 0 has printed and left)
                if seen is not None or self.rank != 0:
                    os._exit(SIDE_LINE_RC)
            if seen is not None and time.time() - seen > 60:
                os._exit(SIDE_LINE_RC)

    def fail(self, exc):
        err = "rank %d: %s" % (self.rank, exc if isinstance(exc, SystemExit) else repr(exc))
        log("side line %s failed: %s" % (self.phase, err))
        if self.rank == 0:
            self._emit_and_exit(err)
        try:
            self.store.set(self.KEY_ERR, err)
        except Exception:  # noqa: BLE001
            os._exit(SIDE_LINE_RC)
        time.sleep(120)  # the watchdog leaves once rank 0 has printed
        os._exit(SIDE_LINE_RC)

    def finish(self):
        """Normal end: rank 0 prints the line (the watchdog can no longer)."""
        with self.lock:
            if self.printed:
                os._exit(SIDE_LINE_RC)  # pragma: no cover (the watchdog printed and is exiting)
            self.printed = True
            if self.rank == 0:
                print(json.dumps(self.res), flush=True)


class SideLines:
    """Runs the side lines after the headline and prints the job's one JSON line.
    A side line that fails is recorded under its key and in the top-level
    `side_line_errors` list; `finish()` returns SIDE_LINE_RC then, else 0.  At
    N > 1 the lines run under SideLineGuard (a raise or stall on one rank)."""

    def __init__(self, dist, rank, res, budget_s=300.0):
        self.rank, self.res = rank, res
        self.guard = SideLineGuard(dist, rank, res, budget_s) if dist is not None else None

    def run(self, key, fn):
        if self.guard is not None:
            self.guard.start(key)
        try:
            self.res[key] = fn()
        except SystemExit as exc:
            # parity checks agree across ranks (max over ranks) before exiting, so
            # every rank lands here together
            self._error(key, str(exc))
        except Exception as exc:  # noqa: BLE001
            if self.guard is not None:
                self.guard.fail(exc)  # does not return
            self._error(key, repr(exc))  # one process: keep the headline line
        if self.guard is not None:
            self.guard.phase = None
        log("%s: %s" % (key, json.dumps(self.res[key])))

    def _error(self, key, err):
        self.res[key] = {"error": err}
        self.res.setdefault("side_line_errors", []).append({"line": key, "error": err})

    def finish(self):
        if self.guard is not None:
            self.guard.finish()
        elif self.rank == 0:
            print(json.dumps(self.res), flush=True)
        return SIDE_LINE_RC if self.res.get("side_line_errors") else 0


def gc_collect():
    import gc
    gc.collect()
    th.cuda.empty_cache()


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(nproc, argv, grace_s=60.0):
    """`bench.py --gpus N` with N > 1 and no launcher around it: start one fresh
    Python process per GPU running this script with the same arguments and the
    environment torch.distributed.run would give it (RANK = LOCAL_RANK = i,
    WORLD_SIZE = N, MASTER_ADDR 127.0.0.1, a free MASTER_PORT), as the reference's
    multi-GPU example spawns one process per device itself
    (examples/pytorch/graphsage/train_sampling_multi_gpu.py:193-200,336).  This
    process never touches the GPU.  Rank 0 prints the JSON line straight to the
    inherited stdout.  When a rank exits non-zero the others get `grace_s` to
    finish (rank 0 may still be printing a line with side-line errors), then
    their process groups are killed.  Returns the job's status: 0 when every rank
    exited 0, else the status of the first rank that failed (128 + signal for a
    rank killed by a signal)."""
    import signal
    import subprocess
    port = _free_port()
    procs = []

    def kill_all(sig):
        for p in procs:
            if p.poll() is None:
                try:
                    os.killpg(p.pid, sig)
                except ProcessLookupError:
                    pass

    def on_term(signum, _frame):
        kill_all(signal.SIGKILL)
        os._exit(128 + signum)

    signal.signal(signal.SIGTERM, on_term)
    signal.signal(signal.SIGINT, on_term)
    for r in range(nproc):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(nproc),
                   LOCAL_WORLD_SIZE=str(nproc), GROUP_RANK="0", ROLE_RANK=str(r),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), DGLMI_BENCH_LAUNCHED="1")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *argv],
                                      env=env, start_new_session=True))
    print("launcher: %d ranks, pids %s, master 127.0.0.1:%d"
          % (nproc, [p.pid for p in procs], port), file=sys.stderr, flush=True)
    rcs = [None] * nproc
    first = None  # (time, rank) of the first failure
    killed = False
    while any(rc is None for rc in rcs):
        for r, p in enumerate(procs):
            if rcs[r] is None and p.poll() is not None:
                rcs[r] = p.returncode
                if p.returncode != 0 and first is None:
                    first = (time.time(), r)
                    print("launcher: rank %d exited with status %d" % (r, p.returncode),
                          file=sys.stderr, flush=True)
        if first is not None and not killed and time.time() - first[0] > grace_s:
            print("launcher: killing the ranks still running %.0f s after rank %d failed"
                  % (grace_s, first[1]), file=sys.stderr, flush=True)
            kill_all(signal.SIGKILL)
            killed = True
        time.sleep(0.1)
    print("launcher: rank exit statuses %s" % rcs, file=sys.stderr, flush=True)
    if first is None:
        return 0
    rc = rcs[first[1]]
    return 128 - rc if rc < 0 else rc


# the largest per-graph edge count a --same-device rehearsal with N >= 3 may use
SAME_DEVICE_MAX_EDGES = 4_000_000


def same_device_small(args):
    """Whether a --same-device run is small enough for N >= 3 ranks sharing one GPU:
    every graph the ranks build (M1 block, C4, C5) at most SAME_DEVICE_MAX_EDGES edges."""
    return (args.edges_per_gpu * args.gpus <= SAME_DEVICE_MAX_EDGES
            and (args.no_c4 or args.c4_edges <= SAME_DEVICE_MAX_EDGES)
            and (args.no_c5 or args.c5_edges <= SAME_DEVICE_MAX_EDGES))


def launcher_stub(mode, world, rank):
    """Worker body of the launcher's CPU test (``--launcher-stub MODE``): no GPU;
    gloo collectives over the ranks the launcher started, then the same
    side-line / print path as the real run.  MODE: ok | crash<r> (rank r exits 7
    before joining) | side<r> (rank r raises inside a side line)."""
    import torch.distributed as dist
    crash = int(mode[5:]) if mode.startswith("crash") else -1
    side = int(mode[4:]) if mode.startswith("side") else -1
    if rank == crash:
        sys.exit(7)
    if world > 1:
        dist.init_process_group("gloo", timeout=__import__("datetime").timedelta(seconds=60))
    ranks = [None] * world
    info = (rank, int(os.environ.get("LOCAL_RANK", "0")), os.getpid())
    if world > 1:
        dist.all_gather_object(ranks, info)
    else:
        ranks = [info]
    res = {"metric": "launcher-stub", "value": 1.0, "n_gpus": world, "ranks": ranks}
    lines = SideLines(dist if world > 1 else None, rank, res, budget_s=60.0)

    def c4():
        if rank == side:
            raise RuntimeError("injected side-line failure")
        t = th.ones(1)
        if world > 1:
            dist.all_reduce(t)
        return {"value": float(t.item())}
    lines.run("c4", c4)
    rc = lines.finish()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return rc


def measure_exchange(part, x, out_ref, args, dist, cdev, device, edges_total):
    """copy_u_sum with the source rows NOT replicated: each step first fetches
    the halo rows with one all-to-all-v (RCCL over xGMI), then aggregates over
    the local [owned | halo] block.  SURVEY §8(e): the with-exchange line."""
    from dgl import distributed as D
    from dgl import kernel as K
    x_full = th.empty(part.n_inner + part.n_halo, FEAT, device=device)
    x_full[:part.n_inner] = x[part.lo:part.hi]
    send_buf = th.empty(int(part.send_counts.sum()), FEAT, device=device)
    out = th.empty_like(out_ref)
    g = part.gidx()

    def xstep():
        D.halo_exchange_into(x_full, part, None, send_buf)
        K.copy_reduce("sum", g, 0, x_full, out)
    xstep()
    th.cuda.synchronize()
    err = float((out - out_ref).abs().max() / out_ref.abs().max().clamp(min=1e-30))
    err = _max_over_ranks(err, dist, cdev)
    if err > 1e-4:
        raise SystemExit("with-exchange copy_u_sum differs from the replicated one: %g" % err)
    steps = max(1, min(args.steps, 5))
    for _ in range(2):
        xstep()
    el = _timed(xstep, steps, dist, cdev)
    moved = th.tensor([float(part.n_halo) * FEAT * 4], device=cdev, dtype=th.float64)
    halo_max = th.tensor([float(part.n_halo)], device=cdev, dtype=th.float64)
    dist.all_reduce(moved)
    dist.all_reduce(halo_max, op=dist.ReduceOp.MAX)
    ex_el = _timed(lambda: D.halo_exchange_into(x_full, part, None, send_buf), steps, dist, cdev)
    # overlapped: owned-source half of the SpMM while the all-to-all-v is in flight,
    # halo half accumulated in the kernel epilogue (dgl.distributed.aggregate_with_halo)
    x_inner = x[part.lo:part.hi]
    recv = th.empty(part.n_halo, FEAT, device=device)
    tmp = th.empty_like(out)
    out2 = th.empty_like(out)

    def ostep():
        D.aggregate_with_halo(x_inner, part, out2, None, recv, send_buf, tmp)
    ostep()
    th.cuda.synchronize()
    oerr = _max_over_ranks(float((out2 - out_ref).abs().max() / out_ref.abs().max().clamp(min=1e-30)),
                           dist, cdev)
    if oerr > 1e-4:
        raise SystemExit("overlapped with-exchange copy_u_sum differs: %g" % oerr)
    for _ in range(2):
        ostep()
    ov_el = _timed(ostep, steps, dist, cdev)
    return {"value": edges_total * steps / ov_el, "unit": "edges/s",
            "ms_per_step": ov_el * 1e3 / steps,
            "schedule": "halo all-to-all-v overlapped with the owned-source half of the SpMM",
            "sequential_ms_per_step": el * 1e3 / steps,
            "sequential_edges_per_s": edges_total * steps / el,
            "exchange_only_ms": ex_el * 1e3 / steps, "steps": steps,
            "halo_bytes_per_step_all_ranks": float(moved.item()),
            "max_halo_rows_per_rank": int(halo_max.item()),
            "exchange": "all_to_all_single (%s) of halo source rows, then local copy_u_sum"
                        % dist.get_backend(),
            "rel_err_vs_replicated": max(err, oerr)}


def stream_copy_peak(device, nbytes=4 << 30, reps=5):
    """Measured HBM stream rate: the library's float4 device copy
    (DGLMIStreamCopy) of a 4 GiB buffer, (read + write bytes) / time on the
    launch stream -- the access pattern MI355X_MICROARCH.md quotes 6.29 TB/s on."""
    from dgl import _ffi
    a = th.empty(nbytes // 4, dtype=th.float32, device=device)
    b = th.empty_like(a)
    a.fill_(1.0)
    stream = th.cuda.current_stream()
    call = lambda: _ffi.check_call(_ffi.lib().DGLMIStreamCopy(
        ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr()), ctypes.c_int64(a.numel()),
        ctypes.c_void_p(stream.cuda_stream)))
    call()
    s, e = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    s.record(stream)
    for _ in range(reps):
        call()
    e.record(stream)
    th.cuda.synchronize()
    ok = bool(th.equal(a[:1 << 20], b[:1 << 20]))
    ms = s.elapsed_time(e) / reps
    del a, b
    if not ok:
        raise RuntimeError("stream copy check failed")
    return 2 * nbytes / (ms * 1e-3) / 1e9


def measure_update_all(g, x, out_ref, args):
    """End-to-end DGLGraph.update_all(copy_u, sum) through the Python boundary
    (frame lookup, output allocation, autograd Function, ctypes call)."""
    import dgl.function as fn
    g.ndata["h"] = x
    g.update_all(fn.copy_u("h", "m"), fn.sum("m", "h2"))  # builds + caches the device CSRs
    th.cuda.synchronize()
    if not th.equal(g.ndata["h2"], out_ref):
        raise SystemExit("update_all result differs from the direct kernel call")
    steps = max(1, min(args.steps, 10))
    el = _timed(lambda: g.update_all(fn.copy_u("h", "m"), fn.sum("m", "h2")), steps, None, None)
    return {"ms_per_call": el * 1e3 / steps, "edges_per_sec": g.number_of_edges() * steps / el,
            "path": "DGLGraph.update_all(fn.copy_u, fn.sum) incl. output allocation"}


def measure_configs(device, steps=5, warmup=2, budgets=(("c2", 120), ("c3", 300), ("c5", 360)),
                    script=None):
    """The other single-GPU BASELINE configs at N = 1, timed on this box beside the
    headline (scripts/bench_configs.py): C2 arxiv-size copy_u_sum and GraphConv layer,
    C3 Reddit-size fused GATConv forward / forward + backward, C5 RelGraphConv on the
    fused R-GCN entries (checked against the unfused route before it is timed).
    Informational, and isolated: each config runs in a child process of its own under
    a time limit (killed with its process group when it overruns), so an import error,
    a GPU fault or a stall there is recorded under its key and can neither change the
    job's status nor stop the headline line from printing."""
    import signal
    import subprocess
    out = {"steps": steps, "warmup": warmup, "source": "scripts/bench_configs.py, one child "
                                                        "process per config"}
    script = script or os.path.join(ROOT, "scripts", "bench_configs.py")
    for name, budget in budgets:
        t0 = time.time()
        cmd = [sys.executable, script, "--configs", name, "--steps", str(steps),
               "--warmup", str(warmup)]
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             start_new_session=True, cwd=ROOT)
        try:
            so, se = p.communicate(timeout=budget)
            lines = [ln for ln in so.decode(errors="replace").splitlines() if ln.startswith("{")]
            if p.returncode == 0 and lines:
                out[name] = json.loads(lines[-1])
            else:
                out[name] = {"error": "rc %d: %s" % (p.returncode,
                                                     se.decode(errors="replace")[-300:])}
        except subprocess.TimeoutExpired:
            os.killpg(p.pid, signal.SIGKILL)
            p.wait()
            out[name] = {"error": "exceeded %d s" % budget}
        except ValueError as exc:
            out[name] = {"error": "unparsable output: %r" % exc}
        out[name]["wall_s"] = time.time() - t0
        log("configs %s: %s" % (name, json.dumps(out[name])))
    return out


def job_roofline(per_rank, world):
    """The headline line's roofline is the JOB's: the bytes of every rank's launch over
    the slowest rank's kernel time, against N x the HBM peak (N = 1: the launch's own).
    ``per_rank``: one record per rank with kernel_ms, alg_bytes, compulsory_bytes and
    traffic (L2-egress bytes from its PMC passes, or None).

    * ``achieved`` / ``frac``: SURVEY §8(d)'s ALGORITHMIC bytes (indptr, indices, one
      gathered 4F-byte source row per edge, the output) over the kernel time -- the
      contract's figure.  The model counts every edge's row, also the hub rows that L2 /
      the Infinity Cache serve again, so on RMAT it exceeds the HBM peak (frac > 1).
    * ``traffic``: the bytes the PMC counters saw leave L2 for the fabric (FETCH_SIZE
      doubled + WRITE_SIZE, MI355X_MICROARCH.md) -- HBM reads PLUS Infinity-Cache hits, so
      an UPPER bound on HBM bytes; ``l2_egress_GBps`` / ``l2_egress_frac`` are its rate.
    * ``compulsory_*``: every source row once, the LOWER bound on HBM bytes.
    * ``hbm_frac_bounds``: [compulsory_frac, l2_egress_frac] -- the launch's HBM fraction
      lies between them (no counter separates Infinity-Cache hits from HBM reads).

    Returns (roofline dict, L2-egress GB/s or None); per_rank and frac_min ride along at
    N > 1."""
    kmax = max(r["kernel_ms"] for r in per_rank)
    peak = HBM_PEAK_GBPS * world
    alg_bytes = sum(r["alg_bytes"] for r in per_rank)
    compulsory = sum(r["compulsory_bytes"] for r in per_rank)
    alg_gbps = alg_bytes / (kmax * 1e-3) / 1e9
    comp_gbps = compulsory / (kmax * 1e-3) / 1e9
    have = all(r["traffic"] for r in per_rank)
    traffic = sum(r["traffic"] for r in per_rank) if have else None
    egress = traffic / (kmax * 1e-3) / 1e9 if have else None
    roof = {"bound": "hbm", "achieved": alg_gbps, "peak": peak, "unit": "GB/s",
            "frac": alg_gbps / peak, "traffic": traffic,
            "kernel": "k_chunk_reduce + k_chunk_fixup (one copy_u_sum launch pair)",
            "kernel_ms": kmax,
            "achieved_from": ("SURVEY §8(d) algorithmic bytes per launch / HIP-event kernel time%s; "
                              "the model counts the re-reads of hub rows that L2 and the Infinity "
                              "Cache serve, so it can exceed the HBM peak"
                              % ("" if world == 1 else
                                 " (each rank's own row block of the world-size graph, summed "
                                 "over the ranks, over the slowest rank's kernel time, against "
                                 "%d x %g GB/s)" % (world, HBM_PEAK_GBPS))),
            "traffic_note": ("L2 -> fabric bytes per launch (rocprofv3 PMC, this run): HBM reads "
                             "plus Infinity-Cache hits, an upper bound on HBM bytes"
                             if have else "no counters this run"),
            "alg_bytes_per_launch": alg_bytes, "alg_GBps": alg_gbps,
            "l2_egress_GBps": egress, "l2_egress_frac": egress / peak if have else None,
            "compulsory_bytes_per_launch": compulsory, "compulsory_GBps": comp_gbps,
            "compulsory_frac": comp_gbps / peak,
            "hbm_frac_bounds": [comp_gbps / peak, egress / peak] if have else None}
    if world > 1:
        fr = [r for r in per_rank if r["frac"] is not None]
        roof["per_rank"] = per_rank
        roof["frac_min"] = min(r["frac"] for r in fr) if fr else None
    return roof, egress


def check_workload(gidx, x, out, n, n_dst, dist, cdev, device):
    """Correctness spot check on the resident workload (``--full``): a checksum of
    checksums is order-independent up to fp32 rounding (sum over rows of out ==
    sum_u outdeg(u) * X[u]); then 4096 random rows recomputed with torch gathers (fp64)."""
    outdeg = th.bincount(gidx.in_csr.indices.long(), minlength=n).double()
    expect = th.zeros(FEAT, dtype=th.float64, device=device)
    for lo in range(0, n, 1 << 22):  # chunked: x.double() of a 2^26-row table is 34 GB
        hi = min(n, lo + (1 << 22))
        expect += (outdeg[lo:hi, None] * x[lo:hi].double()).sum(0)
    got = out.double().sum(0)
    rel = float(((got - expect).abs().max() / expect.abs().max().clamp(min=1)).item())
    rel = _max_over_ranks(rel, dist, cdev)
    log("checksum-of-checksums rel err %.2e (max over ranks)" % rel)
    if rel > 1e-3:
        raise SystemExit("copy_u_sum checksum mismatch: %g" % rel)
    del outdeg, expect, got
    gen = th.Generator(device=device)
    gen.manual_seed(7)
    rows = th.randint(0, n_dst, (4096,), generator=gen, device=device)
    ip = gidx.in_csr.indptr.long()
    beg, end = ip[rows], ip[rows + 1]
    lens = end - beg
    seg = th.repeat_interleave(th.arange(4096, device=device), lens)
    pos = (th.repeat_interleave(beg - th.cumsum(lens, 0) + lens, lens)
           + th.arange(int(lens.sum()), device=device))
    cols = gidx.in_csr.indices.long()[pos]
    xr = x.double()[cols]
    exact = th.zeros(4096, FEAT, dtype=th.float64, device=device).index_add_(0, seg, xr)
    mass = th.zeros(4096, FEAT, dtype=th.float64, device=device).index_add_(0, seg, xr.abs())
    err = (out[rows].double() - exact).abs()
    bad = _max_over_ranks(float((err > 1e-4 + 1e-6 * mass).any()), dist, cdev)
    if bad > 0:
        raise SystemExit("copy_u_sum row check failed: max err %g" % float(err.max()))
    log("row spot check (4096 rows, fp64 torch gathers): max abs err %.2e" % float(err.max()))


# rows of the timed step's output that --dump-outputs keeps (x FEAT fp32 = 32 MiB), all ranks
DUMP_ROWS = 131072


def dump_sample_rows(n_rows, keep):
    """The rows of an n_rows-row output that --dump-outputs writes: all of them when
    they fit, else a fixed seeded sample, ascending."""
    if n_rows <= keep:
        return np.arange(n_rows, dtype=np.int64)
    return np.sort(np.random.default_rng(20231).choice(n_rows, size=keep, replace=False))


def dump_outputs(directory, out, world, rank):
    """``--dump-outputs DIR``: what the last timed step left in ``out`` (the array a
    caller of copy_u_sum receives), for comparing two builds output for output:
    ``out_rows.npy`` -- fp32 rows of it (dump_sample_rows) -- and ``out_colsum.npy``
    -- the fp64 column sums over ALL its rows, so no row escapes.  At N > 1 every
    rank writes its own row block's pair with a ``.rank<r>`` infix."""
    os.makedirs(directory, exist_ok=True)
    tag = "" if world == 1 else ".rank%d" % rank
    rows = dump_sample_rows(int(out.shape[0]), DUMP_ROWS // world)
    idx = th.from_numpy(rows).to(out.device)
    np.save(os.path.join(directory, "out_rows%s.npy" % tag),
            out.index_select(0, idx).cpu().numpy().astype(np.float32, copy=False))
    colsum = th.zeros(out.shape[1], dtype=th.float64, device=out.device)
    for lo in range(0, int(out.shape[0]), 1 << 22):
        colsum += out[lo:lo + (1 << 22)].double().sum(0)
    np.save(os.path.join(directory, "out_colsum%s.npy" % tag), colsum.cpu().numpy())
    log("outputs of the last timed step written to %s" % directory)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true",
                    help="beside the headline: the workload's correctness checks, the rocprofv3 "
                         "PMC passes, the stream-copy probe, update_all, the CPU baseline, the "
                         "with-exchange / C4 / C5 lines and the C2 / C3 / C5 configs (each can be "
                         "left out with its --no-... option); a plain run sets up, warms up, times "
                         "the steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step computed to DIR/*.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    # rehearsal knobs (small graphs, gloo collectives with every rank on one GPU);
    # the headline run uses the defaults
    ap.add_argument("--edges-per-gpu", type=int, default=EDGES_PER_GPU)
    ap.add_argument("--scale", type=int, default=SCALE)
    ap.add_argument("--dist-backend", default="nccl")
    ap.add_argument("--same-device", action="store_true")
    ap.add_argument("--no-exchange", action="store_true",
                    help="N>1: skip the with-halo-exchange measurement")
    ap.add_argument("--no-update-all", action="store_true",
                    help="N=1: skip the end-to-end DGLGraph.update_all measurement")
    ap.add_argument("--no-pmc", action="store_true",
                    help="N=1: skip the rocprofv3 PMC passes (roofline traffic)")
    ap.add_argument("--no-c4", action="store_true",
                    help="skip the fixed-size C4 (10M / 200M, partitioned, with exchange) line")
    ap.add_argument("--no-configs", action="store_true",
                    help="N=1: skip the informational C2 / C3 / C5 config timings")
    ap.add_argument("--no-c5", action="store_true",
                    help="N>1: skip the partitioned C5 R-GCN line")
    ap.add_argument("--c5-nodes", type=int, default=C5_NODES, help=argparse.SUPPRESS)
    ap.add_argument("--c5-edges", type=int, default=C5_EDGES, help=argparse.SUPPRESS)
    ap.add_argument("--c4-nodes", type=int, default=C4_NODES, help=argparse.SUPPRESS)
    ap.add_argument("--c4-edges", type=int, default=C4_EDGES, help=argparse.SUPPRESS)
    ap.add_argument("--c4-rounds", type=int, default=24,
                    help="label-propagation rounds of the C4 partition")
    ap.add_argument("--c4-slack", type=float, default=0.02,
                    help="C4 partition: parts under (1 + slack) x the average edge load "
                         "(strong scaling waits for the largest part)")
    ap.add_argument("--c4-tau", type=int, default=8,
                    help="C4 hybrid exchange: push a partial sum when a part holds >= tau "
                         "sources of a destination")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--pmc-world", type=int, default=1, help=argparse.SUPPRESS)
    ap.add_argument("--pmc-rank", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--launch-grace", type=float, default=60.0,
                    help="self-launched N > 1: seconds the other ranks get after one fails")
    ap.add_argument("--launcher-stub", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.pmc_child:
        pmc_child(args.pmc_world, args.pmc_rank, args.edges_per_gpu, args.scale)
        return 0
    if args.gpus < 1:
        log("--gpus must be >= 1")
        return 2
    if args.steps < 1 or args.warmup < 0:
        log("--steps must be >= 1 and --warmup >= 0")
        return 2
    if args.same_device and args.gpus >= 3 and not same_device_small(args):
        # three or more processes on one GPU crawl inside rocPRIM's
        # decoupled-look-back sorts at full size (partition_stats 180 s per rank at
        # N = 3); a reduced-size rehearsal of the 8-rank topology is allowed
        log("--same-device is refused for N >= 3 at full size (concurrent look-back sorts "
            "stall); rehearse with --edges-per-gpu, --c4-edges and --c5-edges <= %d"
            % SAME_DEVICE_MAX_EDGES)
        return 2
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        # no launcher around us: start the N ranks ourselves, before any GPU call
        return launch_ranks(args.gpus, sys.argv[1:], args.launch_grace)
    world = int(env_world or "1")
    if world != args.gpus:
        log("WORLD_SIZE=%d from the launcher but --gpus %d" % (world, args.gpus))
        return 2
    rank = int(os.environ.get("RANK", "0"))
    if args.launcher_stub:
        return launcher_stub(args.launcher_stub, world, rank)
    m1 = world == 1 and args.edges_per_gpu == EDGES_PER_GPU and args.scale == SCALE
    pmc = None
    under_profiler = any(k.startswith("ROCPROF") for k in os.environ)
    local = 0 if args.same_device else int(os.environ.get("LOCAL_RANK", "0"))
    if args.full and not args.no_pmc and not under_profiler:
        # counters first, in child processes on this rank's own GPU, before this
        # process touches the GPU (every rank measures its own launch pair)
        t0 = time.time()
        try:
            pmc = pmc_traffic_live(world, rank, local, args.edges_per_gpu, args.scale)
        except Exception as exc:  # the counters must never take the GPU line down
            log("pmc passes failed: %r" % exc)
        trace("pmc passes: %s (%.1fs)" % ("ok" if pmc else "unavailable", time.time() - t0))
        log("pmc passes: %s (%.1fs)" % ("ok" if pmc else "unavailable", time.time() - t0))
    th.cuda.set_device(local)
    device = "cuda:%d" % local
    dist = None
    cdev = device
    if world > 1:
        import torch.distributed as dist
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=th.device(device))
        else:
            dist.init_process_group(args.dist_backend)
            cdev = "cpu"  # gloo collectives on host tensors

    import dgl  # noqa: F401
    from dgl import kernel as K

    n, n_dst, src, dst, x = build_workload(world, rank, device, args.edges_per_gpu, args.scale)
    t0 = time.time()
    gidx, (o_ptr, o_idx) = make_local_graph(n, n_dst, src, dst, device)
    m_local = src.shape[0]
    th.cuda.synchronize()
    log("CSRs built on device in %.2fs" % (time.time() - t0))
    part = None
    if world > 1 and args.full and not args.no_exchange:
        # the same rows planned as a halo partition (owned X rows + halo rows
        # fetched by one all-to-all-v per step), for the with-exchange line
        from dgl import distributed as D
        t0 = time.time()
        bounds = [n * p // world for p in range(world + 1)]
        part = D.build_device_partition(src, dst, bounds, rank)
        part.release_edges()
        th.cuda.synchronize()
        log("halo plan built on device in %.2fs: %d halo rows on rank 0"
            % (time.time() - t0, part.n_halo))
    upd = None
    if world == 1 and args.full and not args.no_update_all:
        import dgl
        upd = dgl.DGLGraph.from_device_coo(src, dst, n)
    del src, dst

    out = th.empty(n_dst, FEAT, device=device)

    def step():
        K.copy_reduce("sum", gidx, 0, x, out)

    step()
    th.cuda.synchronize()
    if args.full:
        check_workload(gidx, x, out, n, n_dst, dist, cdev, device)

    for _ in range(args.warmup):
        step()
    stream = th.cuda.current_stream()
    ev = [(th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True))
          for _ in range(args.steps)]
    if dist is not None:
        dist.barrier()
    th.cuda.synchronize()
    t_start = time.perf_counter()
    for i in range(args.steps):
        ev[i][0].record(stream)
        step()
        ev[i][1].record(stream)
    th.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    th.cuda.synchronize()
    elapsed = time.perf_counter() - t_start
    kernel_ms = float(np.mean([a.elapsed_time(b) for a, b in ev]))
    edges_total = m_local
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, out, world, rank)
    if pmc is None and m1 and args.full:
        # no live counters (profiler unavailable, or this run is itself under
        # rocprofv3): the committed passes of the same launch at this head
        try:
            pmc = dict(json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json"))))
            pmc["source"] = "profiles/pmc_traffic.json (committed rocprofv3 passes, same launch)"
        except (OSError, ValueError):
            pmc = None
    # per-rank launch record: kernel time, edges and the fabric bytes of this rank's
    # own launch pair (its PMC passes) -> its roofline fraction
    # Bytes models per launch of THIS rank's row block, DESIGN.md §6:
    #  * algorithmic: indptr + indices + one gathered 4F-byte source row
    #    per edge + one 4F-byte output row per destination -- counts the re-reads
    #    that L2 serves, so its rate exceeds HBM peak on skewed graphs;
    #  * compulsory: every source row once (the bytes no cache can avoid);
    #  * traffic: what the PMC counters saw leave L2 for the fabric (Infinity
    #    Cache + HBM), measured by this run's own rocprofv3 passes -- an upper bound
    #    on the HBM bytes.  roofline.achieved = algorithmic bytes / kernel time (the
    #    contract); the HBM fraction lies between the compulsory and traffic rates.
    alg_rank = 4 * (n_dst + 1) + 4 * m_local + 4 * FEAT * m_local + 4 * FEAT * n_dst
    comp_rank = 4 * (n_dst + 1) + 4 * m_local + 4 * FEAT * n + 4 * FEAT * n_dst
    per_rank = [{"rank": rank, "kernel_ms": kernel_ms, "edges": int(m_local), "n_dst": int(n_dst),
                 "alg_bytes": int(alg_rank), "compulsory_bytes": int(comp_rank),
                 "traffic": pmc["bytes_per_launch"] if pmc else None,
                 "l2_hit_rate": pmc.get("l2_hit_rate") if pmc else None}]
    if dist is not None:
        t = th.tensor([elapsed], device=cdev, dtype=th.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        k = th.tensor([kernel_ms], device=cdev, dtype=th.float64)
        dist.all_reduce(k, op=dist.ReduceOp.MAX)
        kernel_ms = float(k.item())
        e = th.tensor([m_local], device=cdev, dtype=th.float64)
        dist.all_reduce(e)
        edges_total = int(e.item())
        gathered = [None] * world
        dist.all_gather_object(gathered, per_rank[0])
        per_rank = gathered
    for r in per_rank:
        # the contract's figure (algorithmic bytes) and the L2-egress counter figure
        r["achieved_GBps"] = r["alg_bytes"] / (r["kernel_ms"] * 1e-3) / 1e9
        r["frac"] = r["achieved_GBps"] / HBM_PEAK_GBPS
        r["l2_egress_GBps"] = r["traffic"] / (r["kernel_ms"] * 1e-3) / 1e9 if r["traffic"] else None
        r["l2_egress_frac"] = r["l2_egress_GBps"] / HBM_PEAK_GBPS if r["traffic"] else None

    ms_per_step = elapsed * 1000.0 / args.steps
    value = edges_total * args.steps / elapsed
    upd_res = None
    if upd is not None:
        upd_res = measure_update_all(upd, x, out, args)
        del upd
    roof, egress = job_roofline(per_rank, world)
    if pmc:
        roof["pmc"] = pmc if world == 1 else {k: v for k, v in pmc.items()
                                              if k in ("method", "passes", "fetch_scale")}
    res = {
        "metric": "edges/sec + achieved HBM GB/s, GCN copy_u_sum on 100M-edge graph, 1/2/4/8 MI355X",
        "value": value,
        "unit": "edges/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": ms_per_step,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic RMAT(0.57,0.19,0.19,0.05) generated on device, ids permuted, "
                "X~U(-1,1) seed 2",
        "config": {"workload": "M1 copy_u_sum: RMAT scale %d, %d edges, feat %d, int32 in-CSR%s"
                               % (args.scale + int(round(math.log2(world))), args.edges_per_gpu * world,
                                  FEAT, "" if world == 1 else
                                  ", %d-way dst-row partition, X replicated" % world),
                   "nodes": n, "edges": args.edges_per_gpu * world, "feat": FEAT,
                   "parallelism": "dst-row partition x%d" % world if world > 1 else "single"},
        "roofline": roof,
        # "achieved HBM GB/s" (the metric's second half) is bounded, not measured: the
        # counters see L2 egress (HBM + Infinity Cache), the compulsory bytes are the floor
        "hbm_gbps_bounds": [roof["compulsory_GBps"], egress],
        "edges_per_sec_per_gpu": value / world,
    }
    if not args.full:
        # a plain run: the headline line alone (its roofline from the timed steps' own
        # HIP events and the bytes models; no counters, probes, baselines or side lines)
        if rank == 0:
            print(json.dumps(res), flush=True)
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return 0
    try:
        peak = stream_copy_peak(device)
        res["roofline"]["measured_stream_copy_GBps"] = peak
        res["roofline"]["stream_copy_method"] = ("DGLMIStreamCopy: float4 device copy of a 4 GiB "
                                                 "fp32 buffer, (read + write) / time")
    except RuntimeError as exc:  # out of memory on a crowded device: report, don't fail
        res["roofline"]["measured_stream_copy_GBps"] = None
        log("stream copy peak skipped: %r" % exc)
    if upd_res is not None:
        res["update_all"] = upd_res
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        try:
            res["cpu_baseline"] = cpu_baseline(o_ptr, o_idx, x, n_dst)
        except Exception as exc:  # the baseline must never take the GPU line down
            res["cpu_baseline"] = {"value": None, "error": repr(exc)}
    # Side lines.  At N > 1 they run collectives under the guard, so a rank that
    # fails or stalls in one cannot take the headline line down with it; a failed
    # side line still makes the job's exit status SIDE_LINE_RC.
    lines = SideLines(dist, rank, res)
    if part is not None:
        log("with-exchange line ...")
        lines.run("with_exchange",
                  lambda: measure_exchange(part, x, out, args, dist, cdev, device, edges_total))
    if under_profiler and not args.no_c4:
        # under rocprofv3 the kernel statistics must describe the M1 launch alone
        # (C4 runs the same kernel on a 200 M-edge graph): skip the C4 line
        log("C4 line skipped under the profiler")
    elif not args.no_c4:
        del gidx, o_ptr, o_idx, x, out
        if part is not None:
            del part
        th.cuda.empty_cache()
        lines.run("c4", lambda: measure_c4(world, rank, dist, cdev, device, args))
    if world > 1 and not args.no_c5 and not under_profiler:
        gc_collect()
        lines.run("c5", lambda: measure_c5(world, rank, dist, cdev, device, args))
    if world == 1 and not under_profiler and not args.no_configs:
        gc_collect()
        res["configs"] = measure_configs(device)
    rc = lines.finish()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return rc


if __name__ == "__main__":
    sys.exit(main())
