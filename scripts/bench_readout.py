#!/usr/bin/env python3
"""Times every readout on the segment kernels against the reference's formulation run
with torch on the same device, at F = 64, on two batches:

  small:  65,536 graphs of 8-40 nodes;
  mixed:  the same batch plus one graph of 1 M nodes.

Reference formulations (backend/pytorch/tensor.py:228-239, readout.py:396-432): sum / mean
as ``scatter_add_`` over a segment id, max and softmax by padding every graph to the
largest one (``pad_packed_tensor`` as an index_copy into a (B, L, F) buffer) and
reducing over the pad; the segment id and the pad index are built outside the timed
region, on the device (the reference builds them on the host at every call).  On the
mixed batch the pad would hold B x L x F = 65,537 x 10^6 x 64 floats, so pad + max and
pad + softmax cannot run there and are reported as null.

Each case is timed forward and forward + backward: device events around windows of
about 40 ms of calls (the count chosen per side from a first estimate), the two sides'
windows alternating, the median of `rounds` windows after a warm-up, with the fastest
and slowest window beside it.  Beside the
time: the algorithmic bytes (every input read once, every output written once; backward:
the same for the gradients) over the time, as a fraction of this run's own
DGLMIStreamCopy rate.  Writes profiles/readout_bench.json.

  python scripts/bench_readout.py [--out profiles/readout_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "dgl-hack_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch as th  # noqa: E402

from dgl import _ffi, backend as B, kernel as K  # noqa: E402

F = 64


def window(fn, reps):
    a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def compare(ours, theirs, window_ms, rounds):
    """Per side (theirs may be None): {"ms": median ms per call, "min_ms", "max_ms": the
    spread over the windows, "reps": calls per window}.  Calls per window are chosen per
    side from a first estimate so that a window lasts about `window_ms`; the two sides'
    windows alternate."""
    sides = []
    for fn in (ours, theirs):
        if fn is None:
            sides.append(None)
            continue
        fn()
        fn()
        th.cuda.synchronize()
        est = window(fn, 5)
        sides.append({"fn": fn, "reps": int(min(2000, max(5, np.ceil(window_ms / est)))), "t": []})
    for _ in range(rounds):
        for side in sides:
            if side is not None:
                side["t"].append(window(side["fn"], side["reps"]))
    return [None if side is None else
            {"ms": float(np.median(side["t"])), "min_ms": float(min(side["t"])),
             "max_ms": float(max(side["t"])), "reps": side["reps"]} for side in sides]


def stream_rate(dev, nbytes=1 << 30, reps=10):
    src = th.empty(nbytes // 4, dtype=th.float32, device=dev).normal_()
    dst = th.empty_like(src)
    s = th.cuda.current_stream(dev).cuda_stream
    call = lambda: _ffi.check_call(_ffi.lib().DGLMIStreamCopy(src.data_ptr(), dst.data_ptr(),
                                                              src.numel(), s))
    call()
    th.cuda.synchronize()
    ms = min(window(call, reps) for _ in range(3))
    return 2 * nbytes / (ms * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "readout_bench.json"))
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not th.cuda.is_available():
        raise SystemExit("bench_readout needs the GPU: nothing is timed without one")
    dev = th.device("cuda:0")
    rate = stream_rate(dev)
    rng = np.random.default_rng(0)
    small = rng.integers(8, 41, 65536)
    res = {"device": th.cuda.get_device_name(0), "F": F, "stream_copy_GBps": rate / 1e9,
           "timing": "device events around windows of about %g ms of calls, median (and min, "
                     "max) of %d alternating windows" % (args.window_ms, args.rounds),
           "batches": {}}
    for bname, lens in (("small", small), ("mixed", np.concatenate([small, [1000000]]))):
        off = np.zeros(len(lens) + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        n, nb = int(off[-1]), len(lens)
        seg = K.Segments(th.from_numpy(off).to(dev), n)
        lt = th.from_numpy(np.asarray(lens, np.int64)).to(dev)
        sid = th.repeat_interleave(lt, output_size=n)
        L = int(lens.max())
        can_pad = nb * L * F * 4 <= (8 << 30)
        place = sid * L + (th.arange(n, device=dev) - seg.offsets[sid]) if can_pad else None
        x = th.randn(n, F, device=dev, requires_grad=True)
        w = th.randn(n, device=dev)
        v = th.randn(nb, F, device=dev)
        cnt = lt.clamp(min=1).to(th.float32).unsqueeze(1)
        gB, gN = th.randn(nb, F, device=dev), th.randn(n, F, device=dev)
        idx = sid.unsqueeze(1).expand(n, F)

        def t_sum(feat):
            return th.zeros(nb, F, device=dev).scatter_add_(0, idx, feat)

        def pad(feat, fill):
            return feat.new_full((nb * L, F), fill).index_copy(0, place, feat).view(nb, L, F)

        cases = {
            "sum": (lambda: B.segment_reduce("sum", seg, x), lambda: t_sum(x), gB, n * F + nb * F),
            "mean": (lambda: B.segment_reduce("mean", seg, x), lambda: t_sum(x) / cnt, gB,
                     n * F + nb * F),
            "weighted_sum": (lambda: B.segment_reduce("sum", seg, x, w),
                             lambda: t_sum(x * w.unsqueeze(1)), gB, n * F + n + nb * F),
            "max": (lambda: B.segment_reduce("max", seg, x),
                    (lambda: pad(x, -float("inf")).max(1)[0]) if can_pad else None, gB,
                    n * F + nb * F),
            "softmax": (lambda: B.segment_softmax(seg, x),
                        (lambda: th.softmax(pad(x, -float("inf")), 1).view(nb * L, F)[place])
                        if can_pad else None, gN, 2 * n * F),
            "broadcast": (lambda: B.segment_broadcast(seg, v), lambda: v[sid], None, n * F + nb * F),
        }
        out = {"graphs": nb, "rows": n, "largest": L, "cases": {}}
        for cname, (ours, theirs, gy, floats) in cases.items():
            mine, torch_ = compare(ours, theirs, args.window_ms, args.rounds)
            rec = {"fwd": mine, "torch_fwd": torch_, "fwd_bytes": floats * 4,
                   "fwd_stream_fraction": floats * 4 / (mine["ms"] * 1e-3) / rate,
                   "torch_over_ours_fwd": None if torch_ is None else torch_["ms"] / mine["ms"]}
            if gy is not None:
                def both(fn):
                    def run():
                        x.grad = None
                        fn().backward(gy)
                    return run
                mine, torch_ = compare(both(ours), both(theirs) if theirs else None,
                                       args.window_ms, args.rounds)
                rec.update({"fwd_bwd": mine, "torch_fwd_bwd": torch_,
                            "fwd_bwd_stream_fraction": 2 * floats * 4 / (mine["ms"] * 1e-3) / rate,
                            "torch_over_ours_fwd_bwd":
                                None if torch_ is None else torch_["ms"] / mine["ms"]})
            out["cases"][cname] = rec
            print(bname, cname, json.dumps(rec), flush=True)
        res["batches"][bname] = out
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"wrote": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
