"""Device-resident timing of the exact tail of the enrichment score (libgficf_gsea_exact.so, gficf_gsea_tail_device).

Shape: that of tools/gsea_time.py (G = 20 000 genes, C = 25 clusters, P = 5 000 pathways of 15 to 500 genes, nsim = 1000).  One
call of the sampled enrichment (timed the same way, for the figure beside it) gives the P x C observed scores; the exact call
takes those 125 000 (size, score) pairs.  Times are device events around --iters back-to-back calls after --warmup calls.
"updates" counts m (G - m) per pair, the states of the lattice, whether or not the sweep visits them all: the sweep of a pair
ends with the last step that can block a hit (steps_swept is the share of the G steps it runs, summed over the pairs and
weighted by the registers a lane holds), and a wave carries 64 R >= m + 1 hit indices (lanes_used: (m + 1) / (64 R), weighted
by the steps).
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gsea_time import problem  # noqa: E402


def sweep_model(G: int, size: np.ndarray, es: np.ndarray) -> dict:
    """What the kernel runs, from the closed form of the staircase's last step (x > 0: the last j with m / m - j / (G - m) >= x;
    x < 0: the mirrored walk), without its rounding: wave-steps weighted by R, and the share of their lanes that hold a state."""
    m = size.astype(np.float64)
    jm = np.floor((1.0 - np.abs(es)) * (G - m))
    steps = np.where(es == 0, 0.0, np.minimum(jm + m, G))
    R = 2.0 ** np.ceil(np.log2(np.maximum((m + 1) / 64.0, 1.0)))
    return {"steps_swept": float((steps * R).sum() / (G * R).sum()), "lanes_used": float((steps * (m + 1)).sum() / (steps * 64 * R).sum()),
            "wave_steps_x_R": float((steps * R).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--nsim", type=int, default=1000)
    ap.add_argument("--pathways", type=int, default=5000)
    a = ap.parse_args()
    import torch

    import gficf_amd

    G, C, P = 20000, 25, a.pathways
    stats, ptr, rows = problem(G, C, P, 15, 500)
    size = np.diff(ptr)
    sizes = np.unique(size).astype(np.int32)
    sidx = np.searchsorted(sizes, size).astype(np.int32)
    ops, dev = gficf_amd.HipOps(0), torch.device("cuda", 0)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    d_stats, d_ptr, d_rows, d_sizes, d_sidx = t(stats.T), t(ptr), t(rows), t(sizes), t(sidx)
    ws = torch.empty(ops.gsea_workspace_bytes(G, C, P, len(rows), len(sizes), a.nsim), dtype=torch.uint8, device=dev)
    es, nes, pval = (torch.empty((C, P), dtype=torch.float64, device=dev) for _ in range(3))
    simple = lambda: ops.gsea(G, C, d_stats, d_ptr, d_rows, d_sizes, d_sidx, a.nsim, 180582, ws, es, nes, pval)
    d_size = t(np.tile(size.astype(np.int32), C))                # pair c * P + p, as es is laid out
    d_es = es.reshape(-1)
    tail = torch.empty(C * P, dtype=torch.float64, device=dev)
    ws2 = torch.empty(ops.gsea_tail_workspace_bytes(G, C * P), dtype=torch.uint8, device=dev)
    exact = lambda: ops.gsea_tail(G, d_size, d_es, tail, ws2)

    def timed(run, sync, warmup, iters):
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

    ms_simple = timed(simple, lambda: ops.gsea_sync(ws), 2, 10)
    ms = timed(exact, lambda: ops.gsea_tail_sync(ws2), a.warmup, a.iters)
    m = np.tile(size, C).astype(np.float64)
    updates = float((m * (G - m)).sum())
    h_es, h_tail = es.reshape(-1).cpu().numpy(), tail.cpu().numpy()
    print(json.dumps({"shape": f"G20k_C25_P{P}", "pairs": C * P, "nsim": a.nsim, "simple_ms_per_call": round(ms_simple, 3), "exact_ms_per_call": round(ms, 3),
                      "iters": a.iters, "updates": updates, "updates_per_s": updates / (ms * 1e-3), **sweep_model(G, np.tile(size, C), h_es),
                      "tail_min": float(h_tail.min()), "tail_median": float(np.median(h_tail)), "pval_simple_min": float(pval.min().item())}), flush=True)


if __name__ == "__main__":
    main()
