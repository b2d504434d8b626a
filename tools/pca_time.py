"""Device-resident timing of the randomized SVD (libgficf_pca.so, gficf_rsvd_device) and of its building block Y = A'X.

Shape: the config-3 stand-in, synth.counts_csc(23000, 54000) -> gficf() -> runPCA(dim = 50): k = 50, l = 60, q = 2.
Times are device events around --iters back-to-back calls after --warmup calls:
  rsvd       the whole decomposition (transpose, 2q + 2 = 6 sparse products, 2(2q + 1) + 1 = 11 eigen-solves, the rest);
  tmm_cells  one product A X  (one row per cell:  the genes x cells matrix as it is);
  tmm_genes  one product A'X  (one row per gene: its transpose), layout conversion of the dense operands included.
The kernel split comes from a separate `rocprofv3 --kernel-trace --stats` run of this script (--iters 1 --warmup 0).
--cpu: the numpy port (tests/helpers/rsvd_np.py, LAPACK variant) on the same matrix; run it with OMP_NUM_THREADS=1 for the
single-thread figure.  Prints one JSON line per measurement.
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
    import scipy.sparse as sp
    import torch

    import gficf_amd
    from gficf_amd import synth

    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--genes", type=int, default=23000)
    ap.add_argument("--cells", type=int, default=54000)
    ap.add_argument("--dim", type=int, default=50)
    ap.add_argument("--cpu", action="store_true")
    a = ap.parse_args()
    colptr, rowidx, x = synth.counts_csc(a.genes, a.cells)
    M = gficf_amd.gficf(sp.csc_matrix((x, rowidx, colptr), shape=(a.genes, a.cells)), storeRaw=False, verbose=False)["gficf"]
    G, N = M.shape
    k, q = a.dim, 2
    l = min(k + 10, G, N)
    om = np.random.default_rng(180582).standard_normal((min(G, N), l))
    ops = gficf_amd.HipOps(0)
    dev = torch.device("cuda", 0)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    cp, ri, xv, omd = t(M.indptr.astype(np.int64)), t(M.indices.astype(np.int32)), t(M.data), t(om.T)
    d = torch.empty(k, dtype=torch.float64, device=dev)
    cells = torch.empty((k, N), dtype=torch.float64, device=dev)
    genes = torch.empty((k, G), dtype=torch.float64, device=dev)
    wsb = ops.rsvd_workspace_bytes(G, N, M.nnz, l)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    ms = events(lambda: ops.rsvd(G, N, cp, ri, xv, False, omd, k, l, q, ws, d, cells, genes), lambda: ops.rsvd_sync(ws), a.warmup, a.iters)
    base = {"G": G, "N": N, "nnz": int(M.nnz), "k": k, "l": l, "q": q, "iters": a.iters}
    print(json.dumps({"what": "rsvd", **base, "ms_per_call": round(ms, 3), "ws_GB": round(wsb / 1e9, 2)}), flush=True)
    # the two products by themselves: A X (columns = cells) on M, A'X (columns = genes) on its transpose
    T = gficf_amd.transpose_gficf(M)
    for what, A in (("tmm_cells", M), ("tmm_genes", T)):
        nrows, ncols = A.shape
        acp, ari, ax = t(A.indptr.astype(np.int64)), t(A.indices.astype(np.int32)), t(A.data)
        X = torch.randn((l, nrows), dtype=torch.float64, device=dev)
        Y = torch.empty((l, ncols), dtype=torch.float64, device=dev)
        w2 = torch.empty(ops.csc_tmm_workspace_bytes(nrows, ncols, A.nnz, l), dtype=torch.uint8, device=dev)
        ms = events(lambda: ops.csc_tmm(nrows, ncols, acp, ari, ax, X, l, w2, Y), lambda: ops.rsvd_sync(w2), a.warmup, a.iters)
        gather_gb = A.nnz * 8 * ((l + 7) // 8 * 8) / 1e9
        print(json.dumps({"what": what, **base, "ms_per_call": round(ms, 3), "gathered_GB": round(gather_gb, 1),
                          "gather_TB_per_s": round(gather_gb / ms, 2)}), flush=True)
    if a.cpu:
        from tests.helpers import rsvd_np as rp

        t0 = time.perf_counter()
        rp.rsvd(M, om, k, q, False, "lapack")
        print(json.dumps({"what": "numpy_port", **base, "threads": os.environ.get("OMP_NUM_THREADS", "all"),
                          "s": round(time.perf_counter() - t0, 2)}), flush=True)


if __name__ == "__main__":
    main()
