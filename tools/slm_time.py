"""Device-resident time of gficf_slm_device (graph already in HBM) next to gficf_leiden_device and gficf_louvain_device on the same
matrix, in one process, at the shapes tools/louvain_time.py and tools/leiden_time.py use: config 3 (54 000 cells x k = 30) and
100 000 x 50.  Times are device events around --iters back-to-back calls after --warmup calls of every entry:
  slm 1x1      gficf_slm_device, one start, one iteration: one pass over the levels, to hold against one Leiden iteration
  slm          gficf_slm_device at its defaults (10 starts, up to 10 iterations each)
  leiden       gficf_leiden_device, two iterations
  louvain      gficf_louvain_device, one start, ten iterations
Each call's Q is the library's own; --trace adds one slm 1x1 call with the per-level trace on stderr (GFICF_SLM_DEBUG: vertices,
passes of the local moving and of the sub-moving a level), which says which stage holds the time.  Prints one JSON line a shape.
Usage: python tools/slm_time.py [--shapes N:k,N:k] [--warmup W] [--iters I] [--trace]"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def events(run, warmup: int, iters: int):
    import torch

    out = None
    for _ in range(warmup):
        out = run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        out = run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, out


def run(N, k, warmup, iters, trace):
    import numpy as np
    import torch

    import gficf_amd
    from tools.louvain_time import graph

    _, A = graph(N, k)
    ops = gficf_amd.HipOps(0)
    dev = "cuda:0"
    ptr = torch.from_numpy(A.indptr.astype(np.int64)).to(dev)
    idx = torch.from_numpy(A.indices.astype(np.int32)).to(dev)
    x = torch.from_numpy(A.data).to(dev)
    lab = torch.zeros(N, dtype=torch.int32, device=dev)
    ws_lv = torch.zeros(ops.louvain_workspace_bytes(N, A.nnz, 1), dtype=torch.uint8, device=dev)
    ws_ld = torch.zeros(ops.leiden_workspace_bytes(N, A.nnz), dtype=torch.uint8, device=dev)
    ws_sl = torch.zeros(ops.slm_workspace_bytes(N, A.nnz), dtype=torch.uint8, device=dev)
    calls = {"slm_1x1": lambda: ops.slm(N, ptr, idx, x, 0.8, 1, 1, lab, ws_sl),
             "slm": lambda: ops.slm(N, ptr, idx, x, 0.8, 10, 10, lab, ws_sl),
             "leiden_2": lambda: ops.leiden(N, ptr, idx, x, 0.8, 2, lab, ws_ld),
             "louvain_1": lambda: ops.louvain(N, ptr, idx, x, 0.8, 10, lab, ws_lv, 1, 1, 0)}
    out = {"what": "slm", "N": N, "k": k, "nnz": int(A.nnz), "iters": iters, "ws_MB": round(ws_sl.numel() / 1e6, 1)}
    for name, call in calls.items():
        ms, res = events(call, warmup, iters)
        out[name + "_ms"] = round(ms, 2)
        out[name + "_clusters"], out[name + "_Q"] = int(res[0]), round(float(res[1]), 6)
        if name.startswith("slm"):
            out[name + "_start"], out[name + "_iterations"] = int(res[2]), int(res[3])
    print(json.dumps(out), flush=True)
    if trace:
        os.environ["GFICF_SLM_DEBUG"] = "1"
        calls["slm_1x1"]()
        del os.environ["GFICF_SLM_DEBUG"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="54000:30,100000:50")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    for shape in a.shapes.split(","):
        N, k = (int(v) for v in shape.split(":"))
        run(N, k, a.warmup, a.iters, a.trace)


if __name__ == "__main__":
    main()
