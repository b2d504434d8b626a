"""NumPy restatement of include/gficf_nmf.h, the yardstick of tests/test_nmf_gpu.py: the coordinate-descent solve operation by
operation (a rounded product, then a rounded sum, in the header's order, so the device can be compared in bits), the
half-step around it with the device's chunked column sum, the chain, and the loss on the dense matrix."""
import numpy as np

EPS_H = 1e-15


def nnls_row(S, b, h0=None, cd_tol=1e-8, cd_maxit=100):
    """One row of the solve, exactly as the header words it: (h, sweeps)."""
    k = S.shape[0]
    dg = np.diag(S)
    inv = np.array([1.0 / s if s > 0 else 0.0 for s in dg])
    h = np.zeros(k) if h0 is None else np.where(inv != 0, np.asarray(h0, dtype=np.float64), 0.0)
    g = -np.asarray(b, dtype=np.float64)
    for j in range(k):
        if h[j] != 0:
            g = g + h[j] * S[:, j]
    sweeps = 0
    while sweeps < cd_maxit:
        meas = 0.0
        for j in range(k):
            if inv[j] == 0:
                continue
            x = h[j] - g[j] * inv[j]
            hn = x if x > 0 else 0.0
            dl = hn - h[j]
            if dl != 0:
                g = g + dl * S[:, j]
                h[j] = hn
                meas = max(meas, abs(dl) / (hn + EPS_H))
        sweeps += 1
        if meas < cd_tol:
            break
    return h, sweeps


def nnls_cd(S, B, H0=None, cd_tol=1e-8, cd_maxit=100):
    """The solve for every row of B at once (the rows are independent: the same operations as nnls_row, row by row, on the
    rows still running): (H, sweeps int32)."""
    S, B = np.asarray(S, dtype=np.float64), np.asarray(B, dtype=np.float64)
    M, k = B.shape
    dg = np.diag(S).copy()
    inv = np.zeros(k)
    inv[dg > 0] = 1.0 / dg[dg > 0]
    H = np.zeros((M, k)) if H0 is None else np.where(inv[None, :] != 0, np.asarray(H0, dtype=np.float64), 0.0)
    Gd = -B
    ST = np.ascontiguousarray(S.T)                             # ST[j] = S[:, j]
    for j in range(k):
        idx = np.flatnonzero(H[:, j] != 0)
        if len(idx):
            Gd[idx] = Gd[idx] + H[idx, j][:, None] * ST[j][None, :]
    sweeps = np.zeros(M, dtype=np.int32)
    run = np.arange(M)
    sw = 0
    while sw < cd_maxit and len(run):
        meas = np.zeros(len(run))
        for j in range(k):
            if inv[j] == 0:
                continue
            hj = H[run, j]
            x = hj - Gd[run, j] * inv[j]
            hn = np.where(x > 0, x, 0.0)
            dl = hn - hj
            mv = np.flatnonzero(dl != 0)
            if len(mv):
                rows = run[mv]
                Gd[rows] = Gd[rows] + dl[mv][:, None] * ST[j][None, :]
                H[rows, j] = hn[mv]
                meas[mv] = np.maximum(meas[mv], np.abs(dl[mv]) / (hn[mv] + EPS_H))
        sw += 1
        sweeps[run] = sw
        run = run[~(meas < cd_tol)]
    return H, sweeps


def colsum_chunked(Y):
    """The column sums of Y (m x k) in the order of the library's chunked column sum: at most 256 chunks of rows; in a chunk
    four interleaved running sums (rows r0 + l, r0 + l + 4, ...) added ((s0 + s1) + s2) + s3; the chunks added in order."""
    m, k = Y.shape
    nch = min((max(m, 1) + 255) // 256, 256)
    rpc = (m + nch - 1) // nch
    tot = np.zeros(k)
    for ch in range(nch):
        r0, r1 = ch * rpc, min(ch * rpc + rpc, m)
        s = []
        for l in range(4):
            rows = Y[r0 + l:r1:4] if r0 + l < r1 else Y[:0]
            s.append(np.add.accumulate(rows, axis=0)[-1] if len(rows) else np.zeros(k))
        tot = tot + (((s[0] + s[1]) + s[2]) + s[3])
    return tot


def normalise(Y):
    """(Y with every live column divided by its sum, d, dead): step 3."""
    d = colsum_chunked(Y)
    d = np.where(d > 0, d, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        Yn = np.where(d[None, :] > 0, Y / d[None, :], 0.0)
    return Yn, d, int((d == 0).sum())


def half_step(S, B, Y=None, d=None, cd_tol=1e-8, cd_maxit=100):
    """Steps 2 and 3 from a given S (the ridge in it) and B (the penalty taken off): the solve, warm-started from Y * d, and
    the normalisation: {"y", "d", "sweeps", "dead", "solution"}."""
    H0 = None if Y is None else np.asarray(Y) * np.asarray(d)[None, :]
    H, sweeps = nnls_cd(S, B, H0, cd_tol, cd_maxit)
    Yn, dd, dead = normalise(H)
    return {"y": Yn, "d": dd, "sweeps": sweeps, "dead": dead, "solution": H}


def forms(A, X, l1=0.0, ridge=1e-15):
    """Step 1 in numpy's own summation order: S = X'X + ridge, B = A'X - l1 (A: n_in x n_out, dense or scipy sparse)."""
    S = X.T @ X
    S[np.diag_indices_from(S)] += ridge
    return S, np.asarray(A.T @ X) - l1


def delta_of(W, Wp):
    x, y = W.ravel(), Wp.ravel()
    if x.std() == 0 or y.std() == 0:
        return 1.0
    return 1.0 - np.corrcoef(x, y)[0, 1]


def loss(A, w, d, h):
    """||A - w diag(d) h||_F^2 on the dense matrix."""
    A = np.asarray(A.todense()) if hasattr(A, "todense") else np.asarray(A)
    return float(((A - (w * d[None, :]) @ h) ** 2).sum())


def nmf(A, k, W0, tol=1e-4, maxit=100, L1=(0.0, 0.0), cd_tol=1e-8, cd_maxit=100, ridge=1e-15, track_loss=False, keep=()):
    """The chain; ``keep``: iterations (1-based) after which (w, cells) are recorded in "history"."""
    G, N = A.shape
    At = A.T.tocsc() if hasattr(A, "tocsc") else A.T
    W, H, d = np.array(W0, dtype=np.float64), None, None
    deltas, losses, hist, converged, dead = [], [], {}, False, 0
    it = 0
    while it < maxit:
        S, B = forms(A, W, L1[1], ridge)
        r = half_step(S, B, H, d, cd_tol, cd_maxit)
        H, d = r["y"], r["d"]
        Wp = W
        S, B = forms(At, H, L1[0], ridge)
        r = half_step(S, B, W, d, cd_tol, cd_maxit)
        W, d, dead = r["y"], r["d"], r["dead"]
        it += 1
        deltas.append(delta_of(W, Wp))
        if track_loss:
            losses.append(loss(A, W, d, H.T))
        if it in keep:
            hist[it] = (W.copy(), H * d[None, :])
        if deltas[-1] < tol:
            converged = True
            break
    return {"w": W, "d": d, "h": H.T, "cells": H * d[None, :], "iterations": it, "delta": np.array(deltas), "converged": converged,
            "loss": np.array(losses) if track_loss else None, "dead": dead, "history": hist}
