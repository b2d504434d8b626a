"""Device-resident timing of the embedding (libgficf_umap.so) at the config-3 shape: 54 000 cells x 50 components.

Input: --cells points in --dim dimensions, 30 Gaussian blobs (unit variance, centres N(0, 3^2)) — the shape of data$pca$cells,
not its values.  Times are device events around --iters back-to-back calls after --warmup calls, per stage:
  search   gficf_knn_prepare_device + gficf_knn_search_device with distances (k = 15, euclidean)
  graph    gficf_umap_graph_device on the search's own output
  layout   gficf_umap_layout_device, all n_epochs = 200 sweeps, for tumap (a = b = 1) and umap (a, b of min_dist = 0.01)
and the wall time of one gficf_amd.umap() call (upload, the chain, download of embedding + graph + table) for both.
Prints one JSON line per measurement.
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


def events(run, sync, warmup: int, iters: int) -> float:
    import torch

    for _ in range(warmup):
        run()
    sync()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    sync()
    return e0.elapsed_time(e1) / iters


def main():
    import torch

    import gficf_amd

    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--cells", type=int, default=54000)
    ap.add_argument("--dim", type=int, default=50)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--epochs", type=int, default=200)
    a = ap.parse_args()
    N, d, k = a.cells, a.dim, a.k
    rng = np.random.default_rng(1)
    X = rng.normal(0.0, 3.0, size=(30, d))[np.arange(N) % 30] + rng.standard_normal((N, d))
    Y0 = gficf_amd.umap_init("pca", X, N, 1)
    ops = gficf_amd.HipOps(0)
    dev = torch.device("cuda", 0)
    base = {"N": N, "d": d, "k": k, "n_epochs": a.epochs, "iters": a.iters}
    X_cm = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev)
    pts = torch.zeros((N, ops.knn_dpad(d)), dtype=torch.float32, device=dev)
    kws = torch.empty(ops.knn_workspace_bytes(N, N, k), dtype=torch.uint8, device=dev)
    idx = torch.empty((k, N), dtype=torch.int32, device=dev)
    dist = torch.empty((k, N), dtype=torch.float32, device=dev)

    def search():
        ops.knn_prepare(X_cm, N, d, "euclidean", pts)
        ops.knn_search(pts, N, d, k, "euclidean", 0, N, kws, idx, dist)

    ms = events(search, ops.sync, a.warmup, a.iters)
    print(json.dumps({"what": "search", **base, "ms_per_call": round(ms, 3)}), flush=True)
    cap = 2 * N * k
    gws = torch.empty(ops.umap_graph_workspace_bytes(N, k), dtype=torch.uint8, device=dev)
    rowptr = torch.empty(N + 1, dtype=torch.int64, device=dev)
    col = torch.empty(cap, dtype=torch.int32, device=dev)
    val = torch.empty(cap, dtype=torch.float32, device=dev)
    nnz = torch.zeros(1, dtype=torch.int64, device=dev)
    ms = events(lambda: ops.umap_graph(idx, dist, N, k, gws, rowptr, col, val, nnz), lambda: ops.umap_sync(gws), a.warmup, a.iters)
    longest = int(torch.diff(rowptr).max().item())
    print(json.dumps({"what": "graph", **base, "ms_per_call": round(ms, 3), "nnz": int(nnz.item()), "longest_row": longest,
                      "ws_MB": round(gws.numel() / 1e6, 1)}), flush=True)
    lws = torch.empty(ops.umap_layout_workspace_bytes(N, cap), dtype=torch.uint8, device=dev)
    Y_init = torch.from_numpy(Y0.astype(np.float32)).to(dev)
    Y = Y_init.clone()
    ab = {"tumap": (1.0, 1.0), "umap": gficf_amd.find_ab_params(1.0, 0.01)}
    for name, (ca, cb) in ab.items():
        def layout():
            Y.copy_(Y_init)
            ops.umap_layout(N, rowptr, col, val, cap, ca, cb, 1.0, 1.0, 5, a.epochs, 0, a.epochs, 1, Y, lws)

        ms = events(layout, lambda: ops.umap_sync(lws), a.warmup, a.iters)
        print(json.dumps({"what": "layout_" + name, **base, "ms_per_call": round(ms, 3), "us_per_epoch": round(1e3 * ms / a.epochs, 1)}),
              flush=True)
    for name, (ca, cb) in ab.items():
        gficf_amd.umap(X, Y0, n_neighbors=k, n_epochs=a.epochs, a=ca, b=cb, seed=1)
        t0 = time.perf_counter()
        for _ in range(a.iters):
            gficf_amd.umap(X, Y0, n_neighbors=k, n_epochs=a.epochs, a=ca, b=cb, seed=1)
        print(json.dumps({"what": "host_call_" + name, **base, "ms_per_call": round(1e3 * (time.perf_counter() - t0) / a.iters, 1)}), flush=True)


if __name__ == "__main__":
    main()
