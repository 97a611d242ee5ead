#!/usr/bin/env python
"""Record tests/golden/hub_plan_fetch_sha.json: the SHA-256 of the output and the source
gradient of every case, walk and row width of tests/test_hub_plan_fetch_gpu.py, cold marks
off.  Run it against a library built from the commit before the 32-position fetch (point
DGL_LIBRARY_PATH at the directory of that libdglmi.so) and name the commit:

    DGL_LIBRARY_PATH=/path/to/parent/_lib python scripts/record_hub_plan_fetch_sha.py COMMIT [OUT.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "dgl-hack_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch as th  # noqa: E402

import test_hub_plan_fetch_gpu as T  # noqa: E402
from dgl import _ffi  # noqa: E402
from dgl.graph_index import ImmutableGraphIndex, device_block_gidx  # noqa: E402


def main():
    commit = sys.argv[1]
    out_path = sys.argv[2] if len(sys.argv) > 2 else T.GOLDEN
    for name in ("DGLMI_HUB_DEGREE", "DGLMI_HUB_HOT_DEGREE", "DGLMI_HOT_DEGREE"):
        os.environ.pop(name, None)
    res = {}
    for case in T.CASES:
        deg, rows, cols = T.case_graph(case)
        T.set_gates(lambda k, v: setattr(ImmutableGraphIndex, k, v), deg, marks=False)
        for reverse in (False, True):
            src, dst = (rows, cols) if reverse else (cols, rows)
            g = device_block_gidx(T.N, T.N, src, dst)
            for f in T.feats(case):
                _, _, out, gx = T.run_case(g, f)
                assert g._hub_plans["out" if reverse else "in"] is not None
                res[T.key(case, reverse, f)] = {"out": T.digest(out), "grad": T.digest(gx)}
    th.cuda.synchronize()
    with open(out_path, "w") as fh:
        json.dump({"recorded_with": "a build of commit %s" % commit, "digests": res}, fh,
                  indent=1, sort_keys=True)
        fh.write("\n")
    print("library %s: %d digests -> %s" % (_ffi._lib_path(), len(res), out_path))


if __name__ == "__main__":
    main()
