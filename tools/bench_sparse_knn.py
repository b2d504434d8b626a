"""Device-resident timing of the exact kNN search over sparse GF-ICF cells (libgficf_sparse_knn.so): the records of DESIGN.md
section 21.

Shape: the config-3 stand-in, ``gficf(synth.counts_csc(23000, 54000))``, k = 16, euclidean and cosine.  Times are device events
around --iters back-to-back calls of ``gficf_sparse_knn_device`` (all N queries) after --warmup calls.  Per metric: ms per call;
entry visits (query tiles x stored entries: every tile streams every candidate column once); visits per second; and the LDS
read rate that implies (a visit gathers ``tile_queries`` f32 values of one gene) against the per-CU figure of the
microarchitecture guide, 256 B per clock and CU, at --cus CUs and --ghz GHz.  No threshold: records.  --small: a 1/10 shape for
a rehearsal.  --queries Q: only the first Q cells are queries (the candidates stay all N), to bound a rehearsal's time.  Prints
one JSON line per record.

The time of the tile kernel alone (``k_sk_tiles``) comes from a kernel trace taken in a run of its own:
``tools/trace_py.sh sparse_knn tools/bench_sparse_knn.py --warmup 0 --iters 1``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_svds import timed  # noqa: E402


def main():
    import scipy.sparse as sp
    import torch

    import gficf_amd
    from gficf_amd import synth

    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--queries", type=int, default=0)
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--ghz", type=float, default=2.4)
    a = ap.parse_args()
    G0, N = (2300, 5400) if a.small else (23000, 54000)
    colptr, rowidx, x = synth.counts_csc(G0, N)
    M = gficf_amd.gficf(sp.csc_matrix((x, rowidx, colptr), shape=(G0, N)), normalize=False, verbose=False)["gficf"]
    G, nnz, k = M.shape[0], M.nnz, a.k
    n_q = min(a.queries, N) if a.queries > 0 else N
    shape = gficf_amd.find_nn_sparse_shape(G, N, k)
    tq = shape["tile_queries"]
    ops = gficf_amd.HipOps(0)
    dev = torch.device("cuda", 0)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    cp, ri, xv = t(M.indptr.astype(np.int64)), t(M.indices.astype(np.int32)), t(M.data)
    ws = torch.empty(ops.sparse_knn_workspace_bytes(G, N, nnz, k, n_q), dtype=torch.uint8, device=dev)
    idx = torch.zeros((k, n_q), dtype=torch.int32, device=dev)
    dist = torch.zeros((k, n_q), dtype=torch.float64, device=dev)
    tiles = -(-n_q // tq)
    visits = tiles * nnz
    peak = 256.0 * a.cus * a.ghz * 1e9
    print(json.dumps({"record": "shape", "G": G, "N": N, "nnz": nnz, "entries_per_cell": round(nnz / N, 1), "k": k, "queries": n_q,
                      "tile_queries": tq, "slices": shape["slices"], "tiles": tiles, "entry_visits": visits}), flush=True)
    for metric in ("euclidean", "cosine"):
        ms = timed(lambda: ops.sparse_knn(G, N, cp, ri, xv, k, metric, 0, n_q, ws, idx, dist), lambda: ops.sparse_knn_sync(ws), a.warmup, a.iters)
        lds = visits * tq * 4 / (ms * 1e-3)
        print(json.dumps({"record": metric, "ms_per_call": round(ms, 2), "visits_per_s": float(f"{visits / (ms * 1e-3):.4g}"),
                          "lds_read_TB_per_s": round(lds / 1e12, 2), "lds_read_share_of_peak": round(lds / peak, 3),
                          "first_row": [int(v) for v in idx[:4, 0].cpu().numpy()]}), flush=True)


if __name__ == "__main__":
    main()
