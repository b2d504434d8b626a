"""Device-resident timing of the spectral start (libgficf_spectral.so) at the config-3 shape: 54 000 cells x 50 components, k = 15.

Input: --cells points in --dim dimensions, 30 Gaussian blobs (unit variance, centres N(0, --centre-sd^2)) — the shape of
data$pca$cells, not its values; the fuzzy graph of their exact neighbour table (gficf_umap_graph_device).  --centre-sd 1 keeps the
blobs overlapping: a graph of one component, which is what the solve needs (the count is printed either way).
Times are device events around --iters back-to-back calls after --warmup calls:
  components   gficf_graph_components_device
  one cycle    gficf_spectral_device with max_restarts = 0 (degree, the basis grown to m columns, Rayleigh-Ritz, the residuals): divided
               by its multiplications it bounds one S-multiply at b = 2 with its projections
  solve        gficf_spectral_device at the defaults (tol 1e-4, m 32), with its restarts and multiplications
Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

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
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--cells", type=int, default=54000)
    ap.add_argument("--dim", type=int, default=50)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--centre-sd", type=float, default=1.0)
    ap.add_argument("--m", type=int, default=32)
    a = ap.parse_args()
    N, d, k, m = a.cells, a.dim, a.k, a.m
    rng = np.random.default_rng(1)
    X = rng.normal(0.0, a.centre_sd, size=(30, d))[np.arange(N) % 30] + rng.standard_normal((N, d))
    ops = gficf_amd.HipOps(0)
    dev = torch.device("cuda", 0)
    X_cm = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev)
    pts = torch.zeros((N, ops.knn_dpad(d)), dtype=torch.float32, device=dev)
    kws = torch.empty(ops.knn_workspace_bytes(N, N, k), dtype=torch.uint8, device=dev)
    idx = torch.empty((k, N), dtype=torch.int32, device=dev)
    dist = torch.empty((k, N), dtype=torch.float32, device=dev)
    ops.knn_prepare(X_cm, N, d, "euclidean", pts)
    ops.knn_search(pts, N, d, k, "euclidean", 0, N, kws, idx, dist)
    cap = 2 * N * k
    gws = torch.empty(ops.umap_graph_workspace_bytes(N, k), dtype=torch.uint8, device=dev)
    rowptr = torch.empty(N + 1, dtype=torch.int64, device=dev)
    col = torch.empty(cap, dtype=torch.int32, device=dev)
    val = torch.empty(cap, dtype=torch.float32, device=dev)
    nnz = torch.zeros(1, dtype=torch.int64, device=dev)
    ops.umap_graph(idx, dist, N, k, gws, rowptr, col, val, nnz)
    ops.umap_sync(gws)
    out = {"what": "spectral", "N": N, "d": d, "k": k, "m": m, "iters": a.iters, "nnz": int(nnz.item()),
           "longest_row": int(torch.diff(rowptr).max().item())}
    labels = torch.empty(N, dtype=torch.int32, device=dev)
    cinfo = torch.zeros(2, dtype=torch.int64, device=dev)
    cws = torch.empty(ops.graph_components_workspace_bytes(N), dtype=torch.uint8, device=dev)
    out["components_ms"] = round(events(lambda: ops.graph_components(N, rowptr, col, cap, labels, cinfo, cws), ops.sync, a.warmup, a.iters), 3)
    out["components"], out["rounds"] = (int(v) for v in cinfo.cpu())
    if out["components"] == 1:
        start = torch.from_numpy(rng.standard_normal((N, 2))).to(dev)
        theta, resid = torch.zeros(2, dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.float64, device=dev)
        vec = torch.empty((N, 2), dtype=torch.float64, device=dev)
        info = torch.zeros(4, dtype=torch.int64, device=dev)
        ws = torch.empty(ops.spectral_workspace_bytes(N, cap, 2, m), dtype=torch.uint8, device=dev)
        out["ws_MB"] = round(ws.numel() / 1e6, 1)
        for name, restarts in (("cycle", 0), ("solve", 200)):
            ms = events(lambda: ops.spectral(N, rowptr, col, val, cap, 2, start, 1e-4, m, restarts, ws, theta, resid, vec, info), ops.sync, a.warmup,
                        a.iters)
            _, r, mult, conv = (int(v) for v in info.cpu())
            out[name + "_ms"] = round(ms, 3)
            out[name + "_multiplications"] = mult
            if restarts == 0:
                out["ms_per_block_step"] = round(ms / mult, 4)      # a multiply at b = 2 with its projections, the components included
            else:
                out.update(restarts=r, converged=bool(conv), theta=[float(v) for v in theta.cpu()], residuals=[float(v) for v in resid.cpu()])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
