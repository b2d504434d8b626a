"""Device-resident time of gficf_harmony_device (cells, levels and permutations already in HBM) and of its stages alone, at the
shapes DESIGN.md 24 quotes: 54 000 cells x 50 components with 4 batches, and 200 000 x 50.  The cells are planted types with a
shift per batch (the generator of the quality tests, scaled up); K, theta, lambda, sigma and the limits are runHarmony's defaults.
Times are device events around --iters back-to-back calls after --warmup calls:
  harmony      the whole chain (it waits once a round for the objective, so this is wall time on the stream)
  round        one clustering round of n_blocks = 20 blocks (five launches a block)
  objective, assign, correct   the other stages, one call each
Prints one JSON line a shape.
Usage: python tools/harmony_time.py [--shapes N:d:B,N:d:B] [--warmup W] [--iters I]"""
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


def cells(N, d, B, types=8, seed=1):
    import numpy as np

    r = np.random.default_rng(seed)
    cent, off = 3 * r.standard_normal((types, d)), 1.5 * r.standard_normal((B, d))
    ct, b = r.integers(0, types, N), r.integers(0, B, N)
    return cent[ct] + off[b] + 0.7 * r.standard_normal((N, d)), b


def run(N, d, B, warmup, iters):
    import numpy as np

    import gficf_amd
    from gficf_amd import api

    X, b = cells(N, d, B)
    p = api._harmony_setup(X, b, 2.0, 1.0, 0.1, None, 0.0, 0.05, 10, 20, 1e-5, 1e-4, 10)
    K = p["K"]
    s = api._HarmonyState(p["X"], p["levels"], p["var_start"], K)
    ops, vs = s.ops, p["var_start"]
    start, perm = gficf_amd.harmony_draws(N, K, 200, 180582)
    Y0 = s.up(p["X"][start])
    ops.harmony_normalise(Y0, Y0, s.ws)
    Zcorr, Zc, R, Y, O, E = s.f64(N, d), s.f64(N, d), s.f64(K, N), s.f64(K, d), s.f64(K, s.B), s.f64(K, s.B)
    theta, lamb, permd, obj = s.up(p["theta"]), s.up(p["lamb"]), s.up(perm), s.f64(1)

    def chain():
        return ops.harmony(s.Z, s.levels, vs, theta, lamb, 0.1, Y0, permd, 10, 10, 20, p["n_blocks"], 1e-5, 1e-4, Zcorr, Zc, R, Y, O, E, s.ws)

    out = {"what": "harmony", "N": N, "d": d, "B": s.B, "K": K, "n_blocks": p["n_blocks"], "iters": iters, "ws_MB": round(s.ws.numel() / 1e6, 1)}
    ms, res = events(chain, warmup, iters)
    out.update(harmony_ms=round(ms, 2), iterations=res["iterations"], rounds=res["rounds"], converged=res["converged"],
               ms_per_round=round(ms / max(res["rounds"], 1), 3))
    # the stages alone, on the state the chain left (Zc, R, O, E, Y of its last iteration)
    stages = {"round": lambda: ops.harmony_round(Zc, s.levels, vs, theta, 0.1, permd[0], p["n_blocks"], R, O, E, Y, s.ws),
              "objective": lambda: ops.harmony_objective(Zc, s.levels, vs, Y, R, O, E, theta, 0.1, obj, s.ws),
              "assign": lambda: ops.harmony_assign(Zc, s.levels, vs, Y, 0.1, R, O, E, s.ws),
              "correct": lambda: ops.harmony_correct(s.Z, s.levels, vs, R, lamb, Zcorr, s.ws)}
    for name, call in stages.items():
        out[name + "_ms"] = round(events(call, warmup, iters)[0], 3)
    info = ops.harmony_sync(s.ws)
    out["flat_clusters"] = info["flat_clusters"]
    out["R_MB"] = round(8e-6 * K * N, 1)
    print(json.dumps(out), flush=True)
    assert np.isfinite(Zcorr.cpu().numpy()).all()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="54000:50:4,200000:50:4")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    for shape in a.shapes.split(","):
        N, d, B = (int(v) for v in shape.split(":"))
        run(N, d, B, a.warmup, a.iters)


if __name__ == "__main__":
    main()
