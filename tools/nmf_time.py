"""Device-resident times of libgficf_nmf.so (matrix, factors and workspace already in HBM) at the shape DESIGN.md 25 quotes: the
GF-ICF matrix of synth.counts_csc(23000, 54000), for k = 20 and k = 100.  The start is nmf()'s, default_rng(180582); the limits
are its defaults.  Times are device events around --iters back-to-back calls after --warmup calls:
  half_h       one half-step on the cells' side from the start W0, from zero (Gram, product, solve, column sums)
  half_w       the other side (on the transposed copy), warm-started
  solve_cold   gficf_nnls_device alone on that half-step's S and B, from zero
  solve_warm   the same, started from its own solution (what a late iteration does: one sweep that moves nothing much)
  chain        gficf_nmf_device with maxit = --maxit and tol = 0 (it waits once an iteration, so this is wall time on the stream)
  loss         gficf_nmf_loss_device
Prints one JSON line per k.
Usage: python tools/nmf_time.py [--genes G] [--cells N] [--k 20,100] [--maxit 5] [--warmup W] [--iters I]"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def events(run, warmup: int, iters: int):
    import torch

    out = None
    for _ in range(warmup):
        out = run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        out = run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, out


def run(A, At, k, maxit, warmup, iters):
    import numpy as np

    from gficf_amd import _nmf_lib, api

    G, N = A.shape
    s, t = api._NmfState(A, k), api._NmfState(At, k)
    ops, tc = s.ops, s.tc
    ldk, lpk = _nmf_lib.ld(k), _nmf_lib.lp(k)
    W0 = s.up(api._nmf_pad(np.random.default_rng(180582).random((G, k)), k, "W0"))
    W, H, d = s.zeros(G, ldk), s.zeros(N, ldk), s.zeros(k)
    S, B, sw, counts = s.zeros(lpk, lpk), s.zeros(N, ldk), s.zeros(N, dtype=tc.int32), s.zeros(2, dtype=tc.int64)
    nnz = A.nnz
    out = {"what": "nmf", "G": G, "N": N, "nnz": nnz, "k": k, "iters": iters, "ws_MB": round(s.ws.numel() / 1e6, 1)}

    def half_h():
        ops.nmf_half(G, N, s.colptr, s.rowidx, s.x, nnz, k, W0, H, d, False, 0.0, 1e-15, 1e-8, 100, s.ws, S=S, B=B, sweeps=sw, counts=counts)

    out["half_h_ms"] = round(events(half_h, warmup, iters)[0], 3)
    out["sweeps_cold_mean"], out["sweeps_cold_max"] = round(float(sw.float().mean()), 2), int(sw.max())
    out["capped_rows"] = int(counts[1])
    W.copy_(W0)

    def half_w():
        W.copy_(W0)
        ops.nmf_half(N, G, t.colptr, t.rowidx, t.x, nnz, k, H, W, d.clone(), True, 0.0, 1e-15, 1e-8, 100, t.ws)

    out["half_w_ms"] = round(events(half_w, warmup, iters)[0], 3)
    Hs, sol = s.zeros(N, ldk), s.zeros(N, ldk)
    out["solve_cold_ms"] = round(events(lambda: ops.nnls(k, S, B, None, 1e-8, 100, Hs, sw, s.ws), warmup, iters)[0], 3)
    sol.copy_(Hs)
    out["solve_warm_ms"] = round(events(lambda: ops.nnls(k, S, B, sol, 1e-8, 100, Hs, sw, s.ws), warmup, iters)[0], 3)
    out["sweeps_warm_mean"] = round(float(sw.float().mean()), 2)
    out["zeros_in_solution"] = round(float((sol[:, :k] == 0).double().mean()), 3)
    ms, res = events(lambda: ops.nmf(G, N, s.colptr, s.rowidx, s.x, nnz, k, W0, 0.0, maxit, 0.0, 0.0, 1e-15, 1e-8, 100, False, W, d, H, s.ws), 1,
                     max(1, iters // 4))
    out.update(chain_ms=round(ms, 2), chain_iterations=res["iterations"], ms_per_iteration=round(ms / max(res["iterations"], 1), 2),
               delta_last=float(res["delta"][-1]), dead=res["dead"])
    loss = s.zeros(4)
    out["loss_ms"] = round(events(lambda: ops.nmf_loss(G, N, s.colptr, s.rowidx, s.x, nnz, k, W, d, H, loss, s.ws), warmup, iters)[0], 3)
    ops.nmf_sync(s.ws)
    ops.nmf_sync(t.ws)
    loss = loss.cpu().numpy()
    out["relative_loss"] = float(loss[0] / loss[1])
    print(json.dumps(out), flush=True)
    assert np.isfinite(W.cpu().numpy()).all() and np.isfinite(H.cpu().numpy()).all()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=23000)
    ap.add_argument("--cells", type=int, default=54000)
    ap.add_argument("--k", default="20,100")
    ap.add_argument("--maxit", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=4)
    a = ap.parse_args()
    import scipy.sparse as sp

    import gficf_amd
    from gficf_amd import synth

    colptr, rowidx, x = synth.counts_csc(a.genes, a.cells)
    A = gficf_amd.gficf(sp.csc_matrix((x, rowidx, colptr), shape=(a.genes, a.cells)), normalize=False, verbose=False)["gficf"]
    A.sort_indices()
    At = gficf_amd.transpose_gficf(A)
    for k in (int(v) for v in a.k.split(",")):
        run(A, At, k, a.maxit, a.warmup, a.iters)


if __name__ == "__main__":
    main()
