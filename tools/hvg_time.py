"""Device-resident timing of the highly variable genes (libgficf_hvg.so), stage by stage.

Shape: the config-3 stand-in, the TMM counts per million of ``synth.counts_csc(23000, 54000)`` (``normCounts(M, 2, 0, TRUE)``,
what ``findClusterMarkers`` hands to ``findVarGenes``).
Times are device events around --iters back-to-back calls after --warmup calls.  The moments pass reads every stored entry
twice through the gene-major view the transpose wrote (12 B read, 12 B written and 16 B read per entry): its figure comes
with the bandwidth that makes, and stands beside the transpose alone, which reads and writes the same bytes.  The curve
(b, a) of the distance stage is the one the host entry fits, whose wall time (copies, four synchronisations, the host's
Gauss-Newton and p-values included) is printed last.  --small: a 1/10 shape for a rehearsal.
Prints one JSON line per stage.
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
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    G, N = (2300, 5400) if a.small else (23000, 54000)
    colptr, rowidx, x = synth.counts_csc(G, N)
    M = gficf_amd.normCounts(sp.csc_matrix((x, rowidx, colptr), shape=(G, N)), 2, 0, True, verbose=False)
    G, nnz = M.shape[0], M.nnz
    ops = gficf_amd.HipOps(0)
    dev = torch.device("cuda", 0)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    f64 = lambda n: torch.empty(n, dtype=torch.float64, device=dev)
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    d_col, d_row, d_x = t(M.indptr.astype(np.int64)), t(M.indices.astype(np.int32)), t(M.data)
    ws = torch.empty(ops.hvg_workspace_bytes(G, N, nnz, 20000), dtype=torch.uint8, device=dev)
    mean, sd, var, lx, ly = (f64(G) for _ in range(5))
    nobs, valid, perm, count = i32(G), i32(G), i32(G), i32(1)
    sync = lambda: ops.hvg_sync(ws)
    shape = {"G": G, "N": N, "nnz": nnz}

    tws = torch.empty(ops.csc_transpose_workspace_bytes(G, N), dtype=torch.uint8, device=dev)
    tp, ti, tx = torch.empty(G + 1, dtype=torch.int64, device=dev), i32(nnz), f64(nnz)
    ms_t = timed(lambda: ops.csc_transpose(G, N, d_col, d_row, d_x, tp, ti, tx, tws), ops.sync, a.warmup, a.iters)
    print(json.dumps({"stage": "transpose alone", **shape, "ms_per_call": round(ms_t, 3)}), flush=True)
    ms = timed(lambda: ops.hvg_moments(G, N, d_col, d_row, d_x, ws, mean, sd, var, nobs, lx, ly, valid), sync, a.warmup, a.iters)
    print(json.dumps({"stage": "moments (transpose + one wave per gene)", "ms_per_call": round(ms, 3), "kernel_ms": round(ms - ms_t, 3),
                      "GB_per_s_at_40B_per_entry": round(40 * nnz / ms / 1e6, 1), "valid": int(valid.sum().item())}), flush=True)

    ms = timed(lambda: ops.hvg_order(lx, valid, ws, perm, count), sync, a.warmup, a.iters)
    n = int(count.item())
    k = int(np.floor(0.2 * n))
    print(json.dumps({"stage": "order (radix sort of lx)", "n": n, "k": k, "ms_per_call": round(ms, 3)}), flush=True)
    xs, ys = lx[perm[:n].long()].contiguous(), ly[perm[:n].long()].contiguous()
    w, fit, s = f64(n), f64(n), f64(3)
    ms = timed(lambda: ops.hvg_robust(xs, ys, k, 3, ws, w, fit, s), sync, a.warmup, a.iters)
    print(json.dumps({"stage": "robust local regression (4 fits at n points, 3 medians)", "ms_per_call": round(ms, 3),
                      "point_pairs_per_fit": int(n) * int(k), "s": [float(v) for v in s.cpu()]}), flush=True)
    x0, x1 = float(xs[0].item()), float(xs[-1].item())
    len5, len1 = int(np.floor((x1 - x0) / 0.005 + 1e-10)) + 1, int(np.floor((x1 - x0) / 0.001 + 1e-10)) + 1
    g5, gap, yseq = f64(len5), i32(len5), f64(len5)

    def trusted():
        ops.hvg_gap(xs, x0, 0.005, 0.05, ws, g5, gap)
        ops.hvg_locfit(xs, ys, w, k, g5, ws, yseq)

    ms = timed(trusted, sync, a.warmup, a.iters)
    print(json.dumps({"stage": "gap counts + fit on the 0.005 grid", "grid": len5, "ms_per_call": round(ms, 3)}), flush=True)

    t0 = time.perf_counter()
    host = gficf_amd.var_genes_from_moments(mean.cpu().numpy(), (sd / mean).cpu().numpy())
    wall = (time.perf_counter() - t0) * 1e3
    cvd, idx = f64(n), i32(n)
    ms = timed(lambda: ops.hvg_curve_distance(xs, ys, host["b"], host["a"], x0, len1, ws, cvd, idx), sync, a.warmup, a.iters)
    print(json.dumps({"stage": "curve distance", "grid": len1, "b": host["b"], "a": host["a"], "ms_per_call": round(ms, 3)}), flush=True)
    stats, dens, am = f64(8), f64(512), i32(1)
    ms = timed(lambda: ops.hvg_kde(cvd, ws, stats, dens, am), sync, a.warmup, a.iters)
    print(json.dumps({"stage": "mode (sort, bandwidth, 512 exact sums)", "bw": float(stats[0].item()), "distMid": float(stats[1].item()),
                      "ms_per_call": round(ms, 3)}), flush=True)

    def whole():
        ops.hvg_moments(G, N, d_col, d_row, d_x, ws, mean, sd, var, nobs, lx, ly, valid)
        ops.hvg_order(lx, valid, ws, perm, count)
        ops.hvg_robust(xs, ys, k, 3, ws, w, fit, s)
        trusted()
        ops.hvg_curve_distance(xs, ys, host["b"], host["a"], x0, len1, ws, cvd, idx)
        ops.hvg_kde(cvd, ws, stats, dens, am)

    ms = timed(whole, sync, a.warmup, a.iters)
    print(json.dumps({"stage": "all device stages back to back", "ms_per_call": round(ms, 3)}), flush=True)
    print(json.dumps({"stage": "gficf_hvg_trend_host (steps 2-7, host wall time)", "ms": round(wall, 2), "cdx0": host["cdx0"], "j0": host["j0"],
                      "nls_iter": host["nls_iter"], "genes_fdr_below_0.1": int((host["FDR"] < .1).sum())}), flush=True)


if __name__ == "__main__":
    main()
