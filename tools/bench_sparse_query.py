"""Device-resident timing of the exact kNN of new sparse cells among trained ones (libgficf_sparse_query.so): the records of
DESIGN.md section 23.

Shape: the matrix of tools/bench_sparse_knn.py, ``gficf(synth.counts_csc(23000, 54000))``; its first 53 000 cells are the
training set, its last 1 000 the queries, k = 16, euclidean.  Every call is timed by its own pair of device events, --iters calls
back to back after --warmup calls; a record holds the median, the fastest and the slowest call.  Records:

  * ``query``: ``gficf_sparse_query_device``: ms per call, tiles and slices, entry visits (every tile streams its slice's share of
    the training entries: tiles x nnz_train over all slices) and visits per second;
  * ``range``: ``gficf_sparse_knn_device`` on the stacked matrix for the queries [53000, 54000): the nearest thing the square
    search can do; it streams the same candidates plus the 1 000 queries themselves;
  * ``ratio``: query / range by the medians, next to the range call's own spread (slowest / fastest);
  * the square search's 9.14e11 visits per second over all 54 000 queries for comparison.

No threshold: records.  --small: a 1/10 shape for a rehearsal.  Prints one JSON line per record.

Where the time goes comes from a kernel trace taken in a run of its own:
``tools/trace_py.sh sparse_query tools/bench_sparse_query.py --warmup 0 --iters 1``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SQUARE_VISITS_PER_S = 9.14e11                                  # all 54 000 cells as queries, euclidean


def timed_each(run, sync, warmup: int, iters: int) -> list:
    """ms of each of ``iters`` back-to-back calls, every one between its own two device events."""
    import torch

    for _ in range(warmup):
        run()
    sync()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    marks[0].record()
    for i in range(iters):
        run()
        marks[i + 1].record()
    sync()
    return [marks[i].elapsed_time(marks[i + 1]) for i in range(iters)]


def summary(ms: list) -> dict:
    return {"ms_per_call": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
            "spread": round(max(ms) / min(ms), 3)}


def main():
    import scipy.sparse as sp
    import torch

    import gficf_amd
    from gficf_amd import synth

    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--metric", default="euclidean")
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    G0, n_all, n_new = (2300, 5400, 100) if a.small else (23000, 54000, 1000)
    colptr, rowidx, x = synth.counts_csc(G0, n_all)
    A = gficf_amd.gficf(sp.csc_matrix((x, rowidx, colptr), shape=(G0, n_all)), normalize=False, verbose=False)["gficf"]
    N, k = n_all - n_new, a.k
    train, Q = sp.csc_matrix(A[:, :N]), sp.csc_matrix(A[:, N:])
    G = A.shape[0]
    shape = gficf_amd.find_nn_sparse_query_shape(G, N, n_new, k)
    tq, slices = shape["tile_queries"], shape["slices"]
    tiles = -(-n_new // tq)
    ops = gficf_amd.HipOps(0)
    dev = torch.device("cuda", 0)
    up = lambda B: [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (B.indptr.astype(np.int64), B.indices.astype(np.int32), B.data)]
    d_t, d_q, d_a = up(train), up(Q), up(A)
    idx = torch.zeros((k, n_new), dtype=torch.int32, device=dev)
    dist = torch.zeros((k, n_new), dtype=torch.float64, device=dev)
    print(json.dumps({"record": "shape", "G": G, "N_train": N, "M": n_new, "nnz_train": train.nnz, "nnz_query": Q.nnz, "k": k, "metric": a.metric,
                      "tile_queries": tq, "tiles": tiles, "slices": slices, "workgroups": tiles * slices,
                      "entry_visits": tiles * train.nnz}), flush=True)
    # the query form
    ws = torch.empty(ops.sparse_query_workspace_bytes(G, N, train.nnz, n_new, Q.nnz, k), dtype=torch.uint8, device=dev)
    ms_q = timed_each(lambda: ops.sparse_query(G, N, *d_t, n_new, *d_q, k, a.metric, ws, idx, dist), lambda: ops.sparse_query_sync(ws), a.warmup, a.iters)
    visits = tiles * train.nnz
    rec_q = summary(ms_q)
    print(json.dumps(dict({"record": "query", "visits_per_s": float(f"{visits / (rec_q['ms_per_call'] * 1e-3):.4g}"),
                           "share_of_square_rate": round(visits / (rec_q["ms_per_call"] * 1e-3) / SQUARE_VISITS_PER_S, 3)}, **rec_q,
                          first_row=[int(v) for v in idx[:4, 0].cpu().numpy()])), flush=True)
    # the square search's range form on the stacked matrix
    ws2 = torch.empty(ops.sparse_knn_workspace_bytes(G, n_all, A.nnz, k, n_new), dtype=torch.uint8, device=dev)
    ms_r = timed_each(lambda: ops.sparse_knn(G, n_all, *d_a, k, a.metric, N, n_all, ws2, idx, dist), lambda: ops.sparse_knn_sync(ws2), a.warmup, a.iters)
    rec_r = summary(ms_r)
    visits_r = tiles * A.nnz
    print(json.dumps(dict({"record": "range", "entry_visits": visits_r, "visits_per_s": float(f"{visits_r / (rec_r['ms_per_call'] * 1e-3):.4g}")},
                          **rec_r, first_row=[int(v) for v in idx[:4, 0].cpu().numpy()])), flush=True)
    print(json.dumps({"record": "ratio", "query_over_range": round(rec_q["ms_per_call"] / rec_r["ms_per_call"], 3), "range_spread": rec_r["spread"],
                      "query_spread": rec_q["spread"], "square_visits_per_s": SQUARE_VISITS_PER_S}), flush=True)


if __name__ == "__main__":
    main()
