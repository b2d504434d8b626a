"""Device-resident timing of GSVA (libgficf_gsva.so: gficf_gsva_density_device, gficf_gsva_scores_device).

Shape: the config-3 stand-in, ``synth.counts_csc(23000, 54000)`` with at most 4 096 gene draws per cell (the library's limit of
stored entries per cell), through ``gficf()``; 25 uneven clusters; a hallmark-sized collection (50 pathways of 32-200 genes)
and a C2-sized one (5 000 pathways of 15-500 genes), minSize = 15.
Times are device events around --iters back-to-back calls after --warmup calls, the densities and the scores apart.  The
density figure comes with the number of erfc evaluations the kernel makes (over the kept segments nz * (nz + 1), and nz more
where the segment has zeros), counted from the segment lengths.  --small: a 1/10 shape for a rehearsal.
Prints one JSON line per figure.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def problem(G: int, N: int, C: int, seed: int = 7):
    import scipy.sparse as sp

    import gficf_amd
    from gficf_amd import synth
    from gficf_amd.api import _gsva_args, _gsva_forms

    colptr, rowidx, x = synth.counts_csc(G, N, max_per_cell=4096)
    res = gficf_amd.gficf(sp.csc_matrix((x, rowidx, colptr), shape=(G, N)), normalize=False, verbose=False)
    rng = np.random.default_rng(seed)
    w = rng.dirichlet(np.full(C, 2.0))
    cluster = rng.choice(C, N, p=w).astype(np.int32)
    M, cl, C, _, _, _, _ = _gsva_args(res["gficf"], cluster, [0], [], 1, np.inf, C)
    return M, cl, _gsva_forms(M, cl, C)


def collection(G: int, P: int, lo: int, hi: int, seed: int):
    rng = np.random.default_rng(seed)
    size = rng.integers(lo, hi + 1, P)
    ptr = np.concatenate([[0], np.cumsum(size)]).astype(np.int64)
    return ptr, np.concatenate([rng.choice(G, int(m), replace=False) for m in size]).astype(np.int32)


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

    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    G0, N, C = (2300, 5400, 25) if a.small else (23000, 54000, 25)
    M, cl, (seg_ptr, cell, x, _, colptr, row, src) = problem(G0, N, C)
    G = M.shape[0]
    seg = np.diff(seg_ptr)
    n_c = np.bincount(cl, minlength=C)
    zeros = np.repeat(n_c[None, :], G, axis=0).ravel() > seg                        # segments whose zeros' group is evaluated
    ops = gficf_amd.HipOps(0)
    dev = torch.device("cuda", 0)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    d_cl, d_seg, d_cell, d_x, d_col, d_row, d_src = t(cl), t(seg_ptr), t(cell), t(x), t(colptr), t(row), t(src)
    sd, d0 = (torch.empty((C, G), dtype=torch.float64, device=dev) for _ in range(2))
    kept = torch.empty((C, G), dtype=torch.int32, device=dev)
    dnz = torch.empty(max(len(x), 1), dtype=torch.float64, device=dev)
    shape = {"G": G, "N": N, "C": C, "nnz": int(len(x)), "longest_segment": int(seg.max()), "longest_cell": int(np.diff(colptr).max())}
    ws = torch.empty(ops.gsva_workspace_bytes(G, N, C, 0), dtype=torch.uint8, device=dev)
    ms = timed(lambda: ops.gsva_density(G, N, C, d_cl, d_seg, d_cell, d_x, int(seg.max()), ws, sd, d0, kept, dnz), lambda: ops.gsva_sync(ws), a.warmup,
               a.iters)
    kp = kept.cpu().numpy().T.ravel() != 0                                          # segment g * C + c
    erfc = int((seg[kp] * (seg[kp] + 1)).sum() + seg[kp & zeros].sum())
    print(json.dumps({"stage": "density", **shape, "ms_per_call": round(ms, 3), "erfc_evaluations": erfc, "G_erfc_per_s": round(erfc / ms / 1e6, 1),
                      "kept_pairs": int(kept.sum().item())}), flush=True)
    for name, P, lo, hi in (("hallmark", 50, 32, 200), ("c2", 500 if a.small else 5000, 15, 500)):
        ptr, members = collection(G, P, lo, hi, 11)
        d_ptr, d_mem = t(ptr), t(members)
        ws = torch.empty(ops.gsva_workspace_bytes(G, N, C, P), dtype=torch.uint8, device=dev)
        es = torch.empty((N, P), dtype=torch.float64, device=dev)
        tested = torch.empty((C, P), dtype=torch.int32, device=dev)
        ssum, ssq = (torch.empty((C, P), dtype=torch.float64, device=dev) for _ in range(2))
        run = lambda: ops.gsva_scores(G, N, C, d_cl, d_col, d_row, d_src, shape["longest_cell"], dnz, d0, kept, d_ptr, d_mem, 15, G, 1, ws, es, tested, ssum,
                                      ssq)
        ms = timed(run, lambda: ops.gsva_sync(ws), a.warmup, a.iters)
        pairs = int((tested.sum(dim=1) * torch.from_numpy(n_c).to(dev)).sum().item())
        print(json.dumps({"stage": "scores", "collection": name, "P": P, "members": int(len(members)), "ms_per_call": round(ms, 3),
                          "cell_pathway_walks": pairs, "ns_per_walk": round(ms * 1e6 / max(pairs, 1), 2), "es_MB": round(es.numel() * 8 / 1e6, 1),
                          "es_absmax": float(torch.nan_to_num(es).abs().max().item())}), flush=True)
        del es


if __name__ == "__main__":
    main()
