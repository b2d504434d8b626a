"""Device-resident timing of t-SNE (libgficf_tsne.so): the iteration at 10 000, 54 000 and 200 000 points, and the whole Rtsne call
at the config-3 shape (54 000 cells x 50 components).

Iteration.  P is a made-up symmetric band (every point tied to the 90 points on either side of it, 180 entries per row: the row
length of perplexity 30), the coordinates N(0, 10^2): the cost of an iteration does not depend on the values.  Times are device
events around --iters iterations of gficf_tsne_layout_device after --warmup, and around as many evaluations of
gficf_tsne_gradient_device (the repulsion kernel and the row-local half, without the move).  "Gpairs_per_s" is N^2 / time: the
exact repulsion visits every ordered pair.  "bound_Gpairs_per_s" is the rate the kernel's instruction count allows at the f32
vector peak: 157.3 TFLOPS = 78.6 T lane-operations/s (a fused multiply-add counts two FLOP), 10 issue slots per pair (2 sub,
2 fma, 1 rcp at the issue cost of two, 1 mul, 1 add, 2 fma).

Whole call.  gficf_amd.Rtsne on 30 Gaussian blobs, max_iter = 1000 (upload, search, affinities, layout, KL, download).
Prints one JSON line per measurement."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_LANE_OPS = 157.3e12 / 2
SLOTS_PER_PAIR = 10


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


def band(N: int, half: int = 90):
    off = np.concatenate([np.arange(-half, 0), np.arange(1, half + 1)])
    col = np.sort((np.arange(N)[:, None] + off[None, :]) % N, axis=1).astype(np.int32)
    return np.arange(0, 2 * half * (N + 1), 2 * half, dtype=np.int64), col.ravel(), np.full(2 * half * N, 1.0 / (2 * half * N), dtype=np.float32)


def main():
    import torch

    import gficf_amd

    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="*", default=[10000, 54000, 200000])
    ap.add_argument("--cells", type=int, default=54000, help="the whole call; 0 skips it")
    ap.add_argument("--dim", type=int, default=50)
    ap.add_argument("--max-iter", type=int, default=1000)
    a = ap.parse_args()
    ops = gficf_amd.HipOps(0)
    dev = torch.device("cuda", 0)
    bound = PEAK_LANE_OPS / SLOTS_PER_PAIR / 1e9
    for N in a.sizes:
        ptr, col, val = band(N)
        cap = len(col)
        rowptr, d_col, d_val = torch.from_numpy(ptr).to(dev), torch.from_numpy(col).to(dev), torch.from_numpy(val).to(dev)
        Y = torch.from_numpy((np.random.default_rng(1).standard_normal((N, 2)) * 10).astype(np.float32)).to(dev)
        uY, gains = torch.zeros_like(Y), torch.ones_like(Y)
        dC, zk = torch.empty_like(Y), torch.zeros(2, dtype=torch.float64, device=dev)
        ws = torch.empty(ops.tsne_layout_workspace_bytes(N, cap), dtype=torch.uint8, device=dev)
        shape = gficf_amd.tsne_shape(N)
        base = {"N": N, "nnz": cap, "slices": shape["slices"], "iters": a.iters}
        ms = events(lambda: ops.tsne_gradient(N, rowptr, d_col, d_val, cap, Y, 1.0, ws, dC, None, zk[0:1], None), lambda: ops.tsne_sync(ws),
                    a.warmup, a.iters)
        print(json.dumps({"what": "gradient", **base, "ms_per_call": round(ms, 4), "Gpairs_per_s": round(N * N / ms / 1e6, 1),
                          "bound_Gpairs_per_s": round(bound, 1)}), flush=True)
        n = a.iters
        ms = events(lambda: ops.tsne_layout(N, rowptr, d_col, d_val, cap, n, 0, n, 0, 0, 0.5, 0.8, 200.0, 12.0, Y, uY, gains, ws),
                    lambda: ops.tsne_sync(ws), 1, 1) / n
        print(json.dumps({"what": "iteration", **base, "ms_per_iteration": round(ms, 4), "Gpairs_per_s": round(N * N / ms / 1e6, 1),
                          "bound_Gpairs_per_s": round(bound, 1), "ws_MB": round(ws.numel() / 1e6, 1)}), flush=True)
        del rowptr, d_col, d_val, Y, uY, gains, dC, ws
    if a.cells:
        N, d = a.cells, a.dim
        rng = np.random.default_rng(1)
        X = rng.normal(0.0, 3.0, size=(30, d))[np.arange(N) % 30] + rng.standard_normal((N, d))
        gficf_amd.Rtsne(X, max_iter=2)                                                  # warm: pool, code objects
        t0 = time.perf_counter()
        r = gficf_amd.Rtsne(X, max_iter=a.max_iter)
        print(json.dumps({"what": "Rtsne", "N": N, "d": d, "max_iter": a.max_iter, "s_per_call": round(time.perf_counter() - t0, 3),
                          "kl": round(r["costs"], 4)}), flush=True)


if __name__ == "__main__":
    main()
