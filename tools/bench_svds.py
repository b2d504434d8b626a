"""Device-resident timing of the exact truncated SVD (libgficf_svds.so) beside the randomized one (libgficf_pca.so), and the
deviation of the randomized result from the exact one: the records of DESIGN.md section 20.

Shape: the config-3 stand-in, ``gficf(synth.counts_csc(23000, 54000))``, k = 50, the defaults of ``svds`` (b = 8,
m = min(n, 128), tol = 1e-10) and of ``rsvd`` (p = 10, q = 2).  Times are device events around --iters back-to-back calls after
--warmup calls; ``svds`` waits for the stream once per restart cycle inside, so its figure includes those waits.  In the same
run: two ``csc_tmm`` calls at l = 8, one over the matrix and one over its transposed copy (what one application of the
operator reads), and the ratio of a step of ``svds`` (its time / its products) to them: what of a step the sparse products are.
Deviation: ``d`` of ``rsvd`` against ``d`` of ``svds`` relative to d[0], per component, and the largest principal angle between
the two 50-dimensional ``genes`` subspaces.  No threshold: records.  --small: a 1/10 shape for a rehearsal.  Prints one JSON
line per record.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(run, sync, warmup: int, iters: int) -> float:
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
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    G0, N = (2300, 5400) if a.small else (23000, 54000)
    colptr, rowidx, x = synth.counts_csc(G0, N)
    M = gficf_amd.gficf(sp.csc_matrix((x, rowidx, colptr), shape=(G0, N)), normalize=False, verbose=False)["gficf"]
    G, nnz, n, k, b = M.shape[0], M.nnz, min(M.shape), a.k, 8
    m, l = min(n, 128), min(a.k + 10, n)
    Mt = sp.csc_matrix(M.T)
    ops = gficf_amd.HipOps(0)
    dev = torch.device("cuda", 0)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
    u8 = lambda nb: torch.empty(nb, dtype=torch.uint8, device=dev)
    cp, ri, xv = t(M.indptr.astype(np.int64)), t(M.indices.astype(np.int32)), t(M.data)
    tcp, tri, txv = t(Mt.indptr.astype(np.int64)), t(Mt.indices.astype(np.int32)), t(Mt.data)
    rng = np.random.default_rng(180582)
    start, omega = t(rng.standard_normal((n, b)).T), t(np.random.default_rng(180582).standard_normal((n, l)).T)
    print(json.dumps({"record": "shape", "G": G, "N": N, "nnz": nnz, "k": k, "b": b, "m": m, "l": l}), flush=True)

    ws = u8(ops.svds_workspace_bytes(G, N, nnz, k, b, m))
    d, cells, genes, resid, info = f64(k), f64(k, N), f64(k, G), f64(k), torch.zeros(4, dtype=torch.int64, device=dev)
    ms_svds = timed(lambda: ops.svds(G, N, cp, ri, xv, False, start, k, b, m, 1e-10, 1000, ws, d, cells, genes, resid, info),
                    lambda: ops.svds_sync(ws), a.warmup, a.iters)
    cycles, products, conv, exh = (int(v) for v in info.cpu().numpy())
    print(json.dumps({"record": "svds", "ms_per_call": round(ms_svds, 2), "cycles": cycles, "products": products, "converged": conv,
                      "exhausted": exh, "ms_per_step": round(ms_svds / max(products, 1), 3), "max_residual": float(resid.max().item())}), flush=True)

    rws = u8(ops.rsvd_workspace_bytes(G, N, nnz, l))
    rd, rcells, rgenes = f64(k), f64(k, N), f64(k, G)
    ms_rsvd = timed(lambda: ops.rsvd(G, N, cp, ri, xv, False, omega, k, l, 2, rws, rd, rcells, rgenes), lambda: ops.rsvd_sync(rws), a.warmup, a.iters)
    print(json.dumps({"record": "rsvd (p = 10, q = 2)", "ms_per_call": round(ms_rsvd, 2), "svds_over_rsvd": round(ms_svds / ms_rsvd, 2)}), flush=True)

    X1, Y1, Y2 = t(rng.standard_normal((b, G))), f64(b, N), f64(b, G)
    w1, w2 = u8(ops.csc_tmm_workspace_bytes(G, N, nnz, b)), u8(ops.csc_tmm_workspace_bytes(N, G, nnz, b))

    def two():
        ops.csc_tmm(G, N, cp, ri, xv, X1, b, w1, Y1)
        ops.csc_tmm(N, G, tcp, tri, txv, Y1, b, w2, Y2)

    ms_two = timed(two, lambda: (ops.rsvd_sync(w1), ops.rsvd_sync(w2)), a.warmup, a.iters)
    print(json.dumps({"record": "two csc_tmm at l = 8 (one application of the operator)", "ms": round(ms_two, 3),
                      "GB_per_s": round(24 * nnz / ms_two / 1e6, 1), "step_over_products": round(ms_svds / max(products, 1) / ms_two, 2)}), flush=True)

    de, dr = d.cpu().numpy(), rd.cpu().numpy()
    Ve, Vr = genes.cpu().numpy().T, rgenes.cpu().numpy().T
    cosines = np.linalg.svd(Ve.T @ Vr, compute_uv=False)
    dev_d = np.abs(dr - de) / de[0]
    print(json.dumps({"record": "rsvd(q = 2) against svds", "d_dev_max": float(dev_d.max()), "d_dev_first_above_1e-6": int(np.argmax(dev_d > 1e-6)) if (dev_d > 1e-6).any() else None,
                      "d_dev_per_component": [float(f"{v:.2e}") for v in dev_d],
                      "largest_principal_angle_rad": float(np.arccos(np.clip(cosines.min(), -1.0, 1.0)))}), flush=True)


if __name__ == "__main__":
    main()
