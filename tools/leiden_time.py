"""Device-resident time of gficf_leiden_device (graph already in HBM) next to gficf_louvain_device with one start on the same matrix, in the
same session, at the shapes tools/louvain_time.py uses: config 3 (54 000 cells x k = 30) and 100 000 x 50.  Louvain with one start is the
yardstick because it does the same local moving without the refinement; Leiden's extra time is the refinement plus the extra levels.
Usage: python tools/leiden_time.py [N k [reps]] ...   (no arguments: both shapes).  LT_DEBUG=1: one more call with the library's per-level trace."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import gficf_amd
from oracle import oracle_np
from tools.louvain_time import graph


def timed(call, lab, reps):
    ts, labs, out = [], [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
        labs.append(lab.cpu().numpy().copy())
    return ts, labs, out


def run(N, k, reps=7):
    _, A = graph(N, k)
    ops = gficf_amd.HipOps(0)
    dev = "cuda:0"
    ptr = torch.from_numpy(A.indptr.astype(np.int64)).to(dev)
    idx = torch.from_numpy(A.indices.astype(np.int32)).to(dev)
    x = torch.from_numpy(A.data).to(dev)
    lab = torch.zeros(N, dtype=torch.int32, device=dev)
    ws_lv = torch.zeros(ops.louvain_workspace_bytes(N, A.nnz, 1), dtype=torch.uint8, device=dev)
    ws_ld = torch.zeros(ops.leiden_workspace_bytes(N, A.nnz), dtype=torch.uint8, device=dev)
    calls = {"louvain_device (1 start, n_iter 10)": lambda: ops.louvain(N, ptr, idx, x, 0.8, 10, lab, ws_lv, 1, 1, 0),
             "louvain_device (1 start, n_iter 2)": lambda: ops.louvain(N, ptr, idx, x, 0.8, 2, lab, ws_lv, 1, 1, 0),
             "leiden_device (n_iterations 2)": lambda: ops.leiden(N, ptr, idx, x, 0.8, 2, lab, ws_ld)}
    for _ in range(2):                               # both warm before either is timed
        for call in calls.values():
            call()
    for name, call in calls.items():
        ts, labs, (nc, q) = timed(call, lab, reps)
        same = all(np.array_equal(labs[0], l) for l in labs[1:])
        qn = oracle_np.modularity_np(A, labs[0], 0.8)
        print(f"{name} N={N} k={k} nnz={A.nnz}: {min(ts):.2f} ms min, {sorted(ts)[len(ts) // 2]:.2f} ms median, {max(ts):.2f} ms max of {reps} "
              f"({nc} clusters, Q {q:.6f}, numpy Q {qn:.6f}, reproducible {same})", flush=True)
    if os.environ.get("LT_DEBUG"):
        os.environ["GFICF_LEIDEN_DEBUG"] = "1"
        calls["leiden_device (n_iterations 2)"]()
        del os.environ["GFICF_LEIDEN_DEBUG"]


if __name__ == "__main__":
    a = sys.argv[1:]
    if not a:
        run(54000, 30)
        run(100000, 50)
    while a:
        run(int(a[0]), int(a[1]), int(a[2]) if len(a) > 2 else 7)
        a = a[3:]
