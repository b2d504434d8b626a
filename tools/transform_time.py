"""Device-resident timing of the transform of new cells (libgficf_transform.so): M new cells against N trained ones.

Input: --cells training points in --dim dimensions, 30 Gaussian blobs (unit variance, centres N(0, 3^2)) — the shape of
data$pca$cells, not its values — a trained plane of the same blobs in 2-D, and queries drawn from the same blobs.  Times are
device events around --iters back-to-back calls after --warmup calls:
  search M     gficf_transform_search_device, k = 15, euclidean, for M in 256, 4 096 and N; with the number of slices S.  At
               M = 256 also with S forced (GFICF_TRANSFORM_SPLIT) to 1, 16 and 64; at M = N the library's square search in its
               plain form (GFICF_KNN_PRUNE=0) in the same run, for comparison
  stages M     memberships, initial positions and the one-launch layout (67 epochs, both curves) for M in 256 and 4 096
and the wall time of one gficf_amd.umap_transform() call.  Prints one JSON line per measurement.
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

from tools.umap_time import events  # noqa: E402


def main():
    import torch

    import gficf_amd

    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--dim", type=int, default=50)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--epochs", type=int, default=67)
    a = ap.parse_args()
    N, d, k = a.cells, a.dim, a.k
    rng = np.random.default_rng(1)
    centres, plane = rng.normal(0.0, 3.0, size=(30, d)), rng.normal(0.0, 8.0, size=(30, 2))
    lab = np.arange(N) % 30
    X = centres[lab] + rng.standard_normal((N, d))
    Yt = (plane[lab] + rng.standard_normal((N, 2))).astype(np.float32)
    ops = gficf_amd.HipOps(0)
    dev = torch.device("cuda", 0)
    base = {"N": N, "d": d, "k": k}
    pts = torch.zeros((N, ops.knn_dpad(d)), dtype=torch.float32, device=dev)
    ops.knn_prepare(torch.from_numpy(np.ascontiguousarray(X.T)).to(dev), N, d, "euclidean", pts)
    d_Yt = torch.from_numpy(Yt).to(dev)
    ab = {"tumap": (1.0, 1.0), "umap": gficf_amd.find_ab_params(1.0, 0.01)}
    for M in (256, 4096, N):
        qry = pts if M == N else pts[rng.permutation(N)[:M]].contiguous() + 0.01       # (near trained points, not on them)
        idx = torch.empty((k, M), dtype=torch.int32, device=dev)
        dist = torch.empty((k, M), dtype=torch.float32, device=dev)
        for force in ([None, 1, 16, 64] if M == 256 else [None]):
            if force is None:
                os.environ.pop("GFICF_TRANSFORM_SPLIT", None)
            else:
                os.environ["GFICF_TRANSFORM_SPLIT"] = str(force)
            sws = torch.empty(ops.transform_workspace_bytes("search", M, N, k), dtype=torch.uint8, device=dev)
            ms = events(lambda: ops.transform_search(pts, N, qry, M, d, k, "euclidean", sws, idx, dist), lambda: ops.transform_sync(sws),
                        a.warmup, a.iters)
            print(json.dumps({"what": "search", **base, "M": M, "S": ops.transform_search_split(M, N), "forced": force is not None,
                              "ms_per_call": round(ms, 3), "ws_MB": round(sws.numel() / 1e6, 1)}), flush=True)
        os.environ.pop("GFICF_TRANSFORM_SPLIT", None)
        if M == N:
            os.environ["GFICF_KNN_PRUNE"] = "0"
            kws = torch.empty(ops.knn_workspace_bytes(N, N, k), dtype=torch.uint8, device=dev)
            i2, d2 = torch.empty_like(idx), torch.empty_like(dist)
            ms = events(lambda: ops.knn_search(pts, N, d, k, "euclidean", 0, N, kws, i2, d2), ops.sync, a.warmup, a.iters)
            os.environ.pop("GFICF_KNN_PRUNE", None)
            print(json.dumps({"what": "square_search_plain", **base, "M": M, "ms_per_call": round(ms, 3),
                              "same_bits": bool(torch.equal(i2, idx) and torch.equal(d2, dist))}), flush=True)
            continue
        w = torch.empty((k, M), dtype=torch.float32, device=dev)
        Y0 = torch.empty((M, 2), dtype=torch.float32, device=dev)
        Y = torch.empty_like(Y0)
        ws = torch.empty(ops.transform_workspace_bytes("layout", M, k=k), dtype=torch.uint8, device=dev)
        sync = lambda: ops.transform_sync(ws)  # noqa: E731
        ms = events(lambda: ops.transform_weights(idx, dist, N, M, k, ws, w), sync, a.warmup, a.iters)
        print(json.dumps({"what": "weights", **base, "M": M, "ms_per_call": round(ms, 3)}), flush=True)
        ms = events(lambda: ops.transform_init(idx, w, d_Yt, N, M, k, ws, Y0), sync, a.warmup, a.iters)
        print(json.dumps({"what": "init", **base, "M": M, "ms_per_call": round(ms, 3)}), flush=True)
        for name, (ca, cb) in ab.items():
            def layout():
                Y.copy_(Y0)
                ops.transform_layout(idx, w, d_Yt, N, M, k, ca, cb, 1.0, 0.25, 5, a.epochs, 0, a.epochs, 1, 0, Y, ws)

            ms = events(layout, sync, a.warmup, a.iters)
            print(json.dumps({"what": "layout_" + name, **base, "M": M, "n_epochs": a.epochs, "ms_per_call": round(ms, 3),
                              "us_per_epoch": round(1e3 * ms / a.epochs, 2)}), flush=True)
    M = 4096
    Q = X[rng.permutation(N)[:M]] + 0.01
    model = {"embedding": Yt.astype(np.float64), "a": 1.0, "b": 1.0, "n_neighbors": k, "metric": "euclidean", "n_epochs": 3 * a.epochs, "seed": 1}
    gficf_amd.umap_transform(Q, model, X)
    t0 = time.perf_counter()
    for _ in range(3):
        gficf_amd.umap_transform(Q, model, X)
    print(json.dumps({"what": "host_call_umap_transform", **base, "M": M, "ms_per_call": round(1e3 * (time.perf_counter() - t0) / 3, 1)}), flush=True)


if __name__ == "__main__":
    main()
