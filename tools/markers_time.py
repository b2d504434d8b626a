"""Device-resident timing of the marker-gene test (libgficf_markers.so, gficf_cluster_markers_device).

Shapes:
  config3  the config-3 stand-in: synth.counts_csc(23000, 54000) scaled to CPM per cell, 25 uneven clusters plus 20
           singletons (45 labels), every gene;
  dense2k  the reference's own call: 2 000 genes of the same CPM matrix, every cluster (findClusterMarkers runs
           rcpp_parallel_WMU_test once per cluster on the dense as.matrix(cpms); here one call covers all of them).
Times are device events around --iters back-to-back calls after --warmup calls.  The kernel split comes from a separate
rocprofv3 --kernel-trace --stats run of this script (--iters 1).  --cpu-genes G: the CPU oracle port (tests/helpers/markers_np.py,
markers_shared: one sort per gene, NumPy, one thread) on G genes of config3, scaled to all genes.
Prints one JSON line per shape.
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


def labels(N: int, seed: int = 3) -> np.ndarray:
    rng = np.random.default_rng(seed)
    sizes = np.maximum((N - 20) * 0.85 ** np.arange(25) * 0.15, 1).astype(np.int64)
    sizes[0] += N - 20 - sizes.sum()
    ids = np.concatenate([np.repeat(np.arange(25), sizes), np.arange(25, 45)]).astype(np.int32)
    rng.shuffle(ids)
    return ids


def cpm_matrix(G: int, N: int):
    import scipy.sparse as sp

    from gficf_amd import synth

    colptr, rowidx, x = synth.counts_csc(G, N)
    M = sp.csc_matrix((x, rowidx, colptr), shape=(G, N))
    M = sp.csc_matrix(M.multiply(1e6 / np.asarray(M.sum(0))))
    M.sort_indices()
    return M


def time_device(M, ids, warmup: int, iters: int) -> dict:
    import torch

    import gficf_amd

    G, N = M.shape
    C = int(ids.max()) + 1
    ops = gficf_amd.HipOps(0)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    colptr, rowidx, x, cl = t(M.indptr.astype(np.int64)), t(M.indices.astype(np.int32)), t(M.data), t(ids)
    wsb = ops.cluster_markers_workspace_bytes(G, N, M.nnz, C)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    p = torch.empty((C, G), dtype=torch.float64, device=dev)
    lfc = torch.empty((C, G), dtype=torch.float64, device=dev)
    run = lambda: ops.cluster_markers(G, N, colptr, rowidx, x, cl, C, ws, p, lfc)
    for _ in range(warmup):
        run()
    ops.cluster_markers_sync(ws)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    ops.cluster_markers_sync(ws)
    ms = e0.elapsed_time(e1) / iters
    return {"G": G, "N": N, "nnz": int(M.nnz), "C": C, "ms_per_call": round(ms, 3), "iters": iters, "ws_GB": round(wsb / 1e9, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--cpu-genes", type=int, default=0)
    ap.add_argument("--shapes", default="config3,dense2k")
    a = ap.parse_args()
    G, N = 23000, 54000
    M = cpm_matrix(G, N)
    ids = labels(N)
    for shape in a.shapes.split(","):
        if shape == "config3":
            r = time_device(M, ids, a.warmup, a.iters)
        else:
            rows = np.argsort(-np.diff(M.tocsr().indptr), kind="stable")[:2000]      # the 2 000 most expressed genes
            r = time_device(M[np.sort(rows)], ids, a.warmup, a.iters)
        print(json.dumps({"shape": shape, **r}), flush=True)
    if a.cpu_genes:
        from tests.helpers import markers_np as mk

        sub = M[: a.cpu_genes]
        t0 = time.perf_counter()
        mk.markers_shared(sub, ids, int(ids.max()) + 1)
        s = time.perf_counter() - t0
        print(json.dumps({"shape": "config3_cpu_oracle", "threads": 1, "genes_timed": a.cpu_genes,
                          "s_scaled_to_all_genes": round(s * G / a.cpu_genes, 1)}), flush=True)


if __name__ == "__main__":
    main()
