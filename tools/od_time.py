"""Device-resident timing of the overdispersed genes (libgficf_od.so), stage by stage.

Shape: the config-3 stand-in, ``gficf(synth.counts_csc(23000, 54000), cell_proportion_min=0.05)``: the raw counts of the kept
genes, their ICF weights and the GF-ICF matrix that ``runPCA(use_odgenes="cr", var_scale="cr")`` selects from and scales.
Times are device events around --iters back-to-back calls after --warmup calls.  ``od_fit`` and ``od_bh_log`` wait for the
stream once inside (the k x k stage and log(n / i) run on the host), so their figures include that wait.  The select-and-scale
pass reads 12 B per stored entry twice and writes 12 B per kept one: its figure comes with the bandwidth that makes.  The host
entry's wall time (copies, the moments, every synchronisation) is printed last.  --small: a 1/10 shape for a rehearsal.
Prints one JSON line per stage.
"""
from __future__ import annotations

import argparse
import json
import math
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
    G0, N = (2300, 5400) if a.small else (23000, 54000)
    colptr, rowidx, x = synth.counts_csc(G0, N)
    data = gficf_amd.gficf(sp.csc_matrix((x, rowidx, colptr), shape=(G0, N)), normalize=False, verbose=False)
    raw, M = data["rawCounts"], data["gficf"]
    G, nnz = M.shape[0], M.nnz
    ops = gficf_amd.HipOps(0)
    dev = torch.device("cuda", 0)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    f64 = lambda n: torch.empty(n, dtype=torch.float64, device=dev)
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    d_col, d_row = t(raw.indptr.astype(np.int64)), t(raw.indices.astype(np.int32))
    d_raw, d_x, d_m = t(raw.data.astype(np.float64)), t(M.data), t(np.asarray(data["w"], dtype=np.float64))
    hws = torch.empty(ops.hvg_workspace_bytes(G, N, nnz, 0), dtype=torch.uint8, device=dev)
    ws = torch.zeros(ops.od_workspace_bytes(G, N), dtype=torch.uint8, device=dev)
    mean, sd, var, lx, ly, v, fit, res, lp, lpa, qv, gsf = (f64(G) for _ in range(12))
    nobs, hvalid, valid = i32(G), i32(G), i32(G)
    sync = lambda: ops.od_sync(ws)
    print(json.dumps({"stage": "shape", "G": G, "N": N, "nnz": nnz}), flush=True)

    ms = timed(lambda: ops.hvg_moments(G, N, d_col, d_row, d_raw, hws, mean, sd, var, nobs, lx, ly, hvalid), lambda: ops.hvg_sync(hws), a.warmup, a.iters)
    print(json.dumps({"stage": "moments of the raw counts (libgficf_hvg.so)", "ms_per_call": round(ms, 3)}), flush=True)
    info = {}
    ms = timed(lambda: info.update(ops.od_fit(d_m, var, nobs, ws, v, valid, fit, res)), sync, a.warmup, a.iters)
    print(json.dumps({"stage": "fit (sort, knots, sums, host k x k stage, fit and res)", "ms_per_call": round(ms, 3), "n": int(info["n"]),
                      "u": int(info["u"]), "basis": int(info["basis"]), "lambda": info["lambda"], "edf": info["edf"]}), flush=True)
    ms = timed(lambda: ops.od_scores(res, nobs, v, N, ws, lp, qv, gsf), sync, a.warmup, a.iters)
    print(json.dumps({"stage": "scores (lp, qv, gsf: one thread per gene)", "ms_per_call": round(ms, 3)}), flush=True)
    ms = timed(lambda: ops.od_bh_log(lp, ws, lpa), sync, a.warmup, a.iters)
    mask = (lpa < math.log(0.1)).to(torch.int32)
    print(json.dumps({"stage": "BH in log space (sort, host log table, running minimum)", "ms_per_call": round(ms, 3),
                      "overdispersed": int(mask.sum().item())}), flush=True)
    ocp, orow, ox, nsel = torch.empty(N + 1, dtype=torch.int64, device=dev), i32(nnz), f64(nnz), i32(1)
    ms = timed(lambda: ops.od_select_scale(G, N, d_col, d_row, d_x, mask, gsf, ws, ocp, orow, ox, nsel), sync, a.warmup, a.iters)
    kept = int(ocp[-1].item())
    print(json.dumps({"stage": "select and scale (count, scan, write)", "ms_per_call": round(ms, 3), "rows": int(nsel.item()), "entries_kept": kept,
                      "GB_per_s": round((24 * nnz + 12 * kept) / ms / 1e6, 1)}), flush=True)
    ms = timed(lambda: ops.od_select_scale(G, N, d_col, d_row, d_x, None, gsf, ws, None, None, ox, None), sync, a.warmup, a.iters)
    print(json.dumps({"stage": "scale only (no mask)", "ms_per_call": round(ms, 3), "GB_per_s": round(20 * nnz / ms / 1e6, 1)}), flush=True)

    def whole():
        ops.hvg_moments(G, N, d_col, d_row, d_raw, hws, mean, sd, var, nobs, lx, ly, hvalid)
        ops.od_fit(d_m, var, nobs, ws, v, valid, fit, res)
        ops.od_scores(res, nobs, v, N, ws, lp, qv, gsf)
        ops.od_bh_log(lp, ws, lpa)
        ops.od_select_scale(G, N, d_col, d_row, d_x, mask, gsf, ws, ocp, orow, ox, nsel)

    ms = timed(whole, sync, a.warmup, a.iters)
    print(json.dumps({"stage": "all device stages back to back", "ms_per_call": round(ms, 3)}), flush=True)
    t0 = time.perf_counter()
    table = gficf_amd.findOverDispersed(data, alpha=0.1, verbose=False)
    wall = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"stage": "findOverDispersed (gficf_od_host, host wall time)", "ms": round(wall, 2),
                      "overdispersed": int((table["lpa"] < math.log(0.1)).sum()), "gsf_zero": int((table["gsf"] == 0).sum())}), flush=True)


if __name__ == "__main__":
    main()
