"""Device-resident timing of the TMM normalisation (libgficf_tmm.so: gficf_tmm_stats_device, gficf_tmm_factors_device,
gficf_tmm_cpm_device).

Shape: the config-3 stand-in, ``synth.counts_csc(23000, 54000)`` (raw counts, as ``gficf()`` hands them to the normalisation
after its gene filter; the filter is not applied here: more genes is the harder case).
Times are device events around --iters back-to-back calls after --warmup calls, the three stages apart.  The factor kernel is
measured against what it has to do at the least: read every stored entry once (12 B: the value and its row) and gather the
reference table (8 B per entry, from L2), so its figure comes with the entries per second and the bandwidth that makes of
20 B per entry; the sort and the searches run in LDS on top of that.  --small: a 1/10 shape for a rehearsal.
Prints one JSON line per stage.
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
    import torch

    import gficf_amd
    from gficf_amd import _tmm_lib, synth

    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    G, N = (2300, 5400) if a.small else (23000, 54000)
    colptr, rowidx, x = synth.counts_csc(G, N)
    nz = np.diff(colptr)
    big = nz > _tmm_lib.LDS_N
    ops = gficf_amd.HipOps(0)
    dev = torch.device("cuda", 0)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    d_col, d_row, d_x = t(colptr), t(rowidx), t(x)
    ws = torch.empty(ops.tmm_workspace_bytes(G, N, int(big.sum()), int(nz[big].sum())), dtype=torch.uint8, device=dev)
    lib, sq, f75, fac = (torch.empty(N, dtype=torch.float64, device=dev) for _ in range(4))
    ostat = torch.empty((2, N), dtype=torch.float64, device=dev)
    gp = torch.empty(1, dtype=torch.int32, device=dev)
    n, kept = (torch.empty(N, dtype=torch.int32, device=dev) for _ in range(2))
    out = torch.empty_like(d_x)
    shape = {"G": G, "N": N, "nnz": int(len(x)), "longest_cell": int(nz.max()), "big_cells": int(big.sum())}
    sync = lambda: ops.tmm_sync(ws)
    ms = timed(lambda: ops.tmm_stats(G, N, d_col, d_row, d_x, int(nz.max()), ws, lib, sq, f75, ostat, gp), sync, a.warmup, a.iters)
    print(json.dumps({"stage": "stats", **shape, "ms_per_call": round(ms, 3), "Gprime": int(gp.item())}), flush=True)
    ref = int(torch.argmax(sq).item()) if float(torch.median(f75).item()) < 1e-20 else int(torch.argmin((f75 - f75.mean()).abs()).item())
    run = lambda: ops.tmm_factors(G, N, d_col, d_row, d_x, int(nz.max()), ref, lib, ws, fac, n, kept, big_cells=int(big.sum()),
                                  big_entries=int(nz[big].sum()))
    ms = timed(run, sync, a.warmup, a.iters)
    print(json.dumps({"stage": "factors", "refColumn": ref, "ms_per_call": round(ms, 3), "common_entries": int(n.sum().item()),
                      "kept_entries": int(kept.sum().item()), "G_entries_per_s": round(len(x) / ms / 1e6, 2),
                      "GB_per_s_at_20B_per_entry": round(20 * len(x) / ms / 1e6, 1)}), flush=True)
    f = fac / torch.exp(torch.log(fac).mean())
    ms = timed(lambda: ops.tmm_cpm(N, d_col, d_x, lib, f, ws, out), sync, a.warmup, a.iters)
    print(json.dumps({"stage": "cpm", "ms_per_call": round(ms, 3), "GB_per_s_at_16B_per_entry": round(16 * len(x) / ms / 1e6, 1),
                      "factor_min": float(f.min().item()), "factor_max": float(f.max().item())}), flush=True)


if __name__ == "__main__":
    main()
