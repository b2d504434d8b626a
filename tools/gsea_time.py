"""Device-resident timing of the gene-set enrichment (libgficf_gsea.so, gficf_gsea_device).

Shape: G = 20 000 genes, C = 25 clusters (|normal| statistics with a 60 % zero tail, as cluster.gene.rnk has), P = 5 000
pathways with sizes drawn uniformly from 15 to 500, nsim = 1000.
Times are device events around --iters back-to-back calls after --warmup calls.  The kernel split comes from a separate
rocprofv3 --kernel-trace --stats run of this script (--iters 1).  --cpu-pathways K: the NumPy oracle (tests/helpers/gsea_np.py:
its null table for the sizes of K pathways, then ES and statistics of those K pathways in every cluster), one thread, scaled
to all P pathways.
Prints one JSON line per figure.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def problem(G: int, C: int, P: int, lo: int, hi: int, seed: int = 7):
    rng = np.random.default_rng(seed)
    stats = np.abs(rng.normal(size=(G, C)))
    stats[rng.random((G, C)) < 0.6] = 0.0
    size = rng.integers(lo, hi + 1, P)
    ptr = np.concatenate([[0], np.cumsum(size)]).astype(np.int64)
    rows = np.concatenate([rng.choice(G, int(m), replace=False) for m in size]).astype(np.int32)
    return stats, ptr, rows


def time_device(stats, ptr, rows, nsim: int, warmup: int, iters: int) -> dict:
    import torch

    import gficf_amd

    G, C = stats.shape
    P = len(ptr) - 1
    size = np.diff(ptr)
    sizes = np.unique(size).astype(np.int32)
    sidx = np.searchsorted(sizes, size).astype(np.int32)
    ops = gficf_amd.HipOps(0)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_stats, d_ptr, d_rows, d_sizes, d_sidx = t(stats.T), t(ptr), t(rows), t(sizes), t(sidx)
    wsb = ops.gsea_workspace_bytes(G, C, P, len(rows), len(sizes), nsim)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    es, nes, pval = (torch.empty((C, P), dtype=torch.float64, device=dev) for _ in range(3))
    run = lambda: ops.gsea(G, C, d_stats, d_ptr, d_rows, d_sizes, d_sidx, nsim, 180582, ws, es, nes, pval)
    for _ in range(warmup):
        run()
    ops.gsea_sync(ws)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    ops.gsea_sync(ws)
    ms = e0.elapsed_time(e1) / iters
    return {"G": G, "C": C, "P": P, "members": int(len(rows)), "D": int(len(sizes)), "nsim": nsim, "ms_per_call": round(ms, 3), "iters": iters,
            "ws_MB": round(wsb / 1e6, 1), "p_min": float(pval.min().item()), "es_max": float(es.max().item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--nsim", type=int, default=1000)
    ap.add_argument("--cpu-pathways", type=int, default=0)
    a = ap.parse_args()
    G, C, P = 20000, 25, 5000
    stats, ptr, rows = problem(G, C, P, 15, 500)
    print(json.dumps({"shape": "G20k_C25_P5k", **time_device(stats, ptr, rows, a.nsim, a.warmup, a.iters)}), flush=True)
    if a.cpu_pathways:
        from tests.helpers import gsea_np as gs

        K = a.cpu_pathways
        t0 = time.perf_counter()
        gs.gsea_np(stats, ptr[:K + 1], rows[:ptr[K]], nsim=a.nsim)
        s = time.perf_counter() - t0
        print(json.dumps({"shape": "G20k_C25_P5k_cpu_oracle", "threads": 1, "pathways_timed": K, "s_scaled_to_all_pathways": round(s * P / K, 1)}),
              flush=True)


if __name__ == "__main__":
    main()
