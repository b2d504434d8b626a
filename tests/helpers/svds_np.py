"""numpy f64 port of the exact truncated SVD of include/gficf_svds.h: block Lanczos with full reorthogonalisation,
Rayleigh-Ritz and thick restart on C = A'A (G <= N) or A A' (N < G), A = t(M) minus its column means when centred.  The
yardstick of tests/test_svds_cpu.py and tests/test_svds_gpu.py: the same block rule, kept count, criterion and finish as the
library, with np.linalg.eigh where the library runs its Jacobi solve and numpy's sums where it adds fixed chunks in order."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from tests.helpers import rsvd_np as rp

MAX_B, MAX_M = 32, 128


def _orth(Y, floor: float = 0.0):
    """orth of rsvd_np (Gram + eigh, twice), directions of the first pass with sqrt(lambda) <= floor dropped as well; the kept
    columns only (they come first)."""
    m = Y.shape[0]
    for p in range(2):
        lam, W = rp._eigh_desc(Y.T @ Y)
        keep = (lam > rp.tau(m) * lam.max()) & (lam > 0)
        if p == 0:
            keep &= np.sqrt(np.where(lam > 0, lam, 0.0)) > floor
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = np.where(keep, 1.0 / np.sqrt(np.where(keep, lam, 1.0)), 0.0)
        Y = Y @ (W * inv)
    return Y[:, :int(keep.sum())]


def check_args(n: int, k: int, b: int, m: int) -> bool:
    return 1 <= b <= MAX_B and b <= m <= min(MAX_M, n) and 1 <= k <= m and (k + 2 * b <= m or m == n)


def schedule(nk: int, n: int, b: int, m: int) -> int:
    """Steps of a cycle that starts with nk kept vectors and takes full-width blocks."""
    cols, steps = nk, 0
    while True:
        cols += min(b, n - cols)
        steps += 1
        if cols >= n or cols + min(b, n - cols) > m:
            return steps


def svds(M_genes_x_cells, start, k: int, m: int | None = None, tol: float = 1e-10, max_cycles: int = 1000, centre: bool = False) -> dict:
    """d (k), cells = U d (N x k), genes = V (G x k), centre, residuals (rho_i / theta_i), converged, cycles, products,
    exhausted.  ``start``: min(N, G) x b."""
    M = sp.csc_matrix(M_genes_x_cells, dtype=np.float64)
    A, At = M.T.tocsr(), M.tocsr()
    N, G = A.shape
    mu = np.asarray(M.sum(axis=1)).ravel() / N if centre else None

    def to_cells(X):
        Y = A @ X
        return Y - (mu @ X)[None, :] if centre else Y

    def to_genes(X):
        Y = At @ X
        return Y - np.outer(mu, X.sum(axis=0)) if centre else Y

    tr = N < G
    to_big, to_small = (to_genes, to_cells) if tr else (to_cells, to_genes)
    n = min(N, G)
    start = np.asarray(start, dtype=np.float64)
    b = start.shape[1]
    m = min(n, MAX_M) if m is None else int(m)
    assert start.shape[0] == n and check_args(n, k, b, m)
    tauv = rp.tau(max(N, G))

    Q = _orth(start)
    V, H = np.zeros((n, 0)), np.zeros((0, 0))
    R = np.zeros((n, 0))
    scale, products, cycles, exhausted, nk = 0.0, 0, 0, Q.shape[1] == 0, 0
    while True:
        cycles += 1
        steps = schedule(nk, n, b, m)
        for s in range(steps):
            if exhausted:
                break
            j0, bwl = V.shape[1], Q.shape[1]
            V = np.hstack([V, Q])
            cols = V.shape[1]
            W = to_small(to_big(Q))
            products += 1
            scale = max(scale, float(np.sqrt((W * W).sum(axis=0)).max()))
            P = V.T @ W
            Hn = np.zeros((cols, cols))
            Hn[:j0, :j0] = H
            Hn[:j0, j0:] = P[:j0]
            Hn[j0:, :j0] = P[:j0].T
            Hn[j0:, j0:] = 0.5 * (P[j0:] + P[j0:].T)
            H = Hn
            W = W - V @ P
            W = W - V @ (V.T @ W)
            R = W
            if cols == n or cols + min(b, n - cols) > m or s == steps - 1:
                exhausted = cols == n
                break
            Q = _orth(W, tauv * scale)[:, :min(b, n - cols)]
            if Q.shape[1] == 0:
                exhausted = True
        cols = V.shape[1]
        if cols:
            theta, Z = rp._eigh_desc(H)
            keep = (theta > tauv * theta.max()) & (theta > 0)
            theta, Z = np.where(keep, theta, 0.0), Z * keep
        else:
            theta, Z = np.zeros(0), np.zeros((0, 0))
        kk = min(k, cols)
        bwl = R.shape[1]
        rho = np.zeros(k)
        if bwl:
            rho[:kk] = np.linalg.norm(R @ Z[cols - bwl:, :kk], axis=0)
        th = np.zeros(k)
        th[:kk] = theta[:kk]
        conv = (rho <= np.maximum(tol * th, tauv * (theta[0] if cols else 0.0)))[:kk]
        if int(conv.sum()) >= k or exhausted or cycles >= max_cycles or m == n:
            break
        nk = min(k + b, cols - b)
        if nk < min(k, cols):
            nk = min(k, cols)
        scale = max(scale, float(theta[0]))
        V = V @ Z[:, :nk]
        H = np.diag(theta[:nk])
        W = R - V @ (V.T @ R)
        W = W - V @ (V.T @ W)
        Q = _orth(W, tauv * scale)[:, :min(b, n - nk)]
        if Q.shape[1] == 0:
            exhausted = True

    Vk = np.zeros((n, k))
    Vk[:, :kk] = V @ Z[:, :kk]
    Vk = Vk @ (1.5 * np.eye(k) - 0.5 * (Vk.T @ Vk))          # one Newton-Schulz step; a zero column stays zero
    T = to_big(Vk)
    d = np.linalg.norm(T, axis=0)
    if tr:
        with np.errstate(divide="ignore", invalid="ignore"):
            genes, cells = np.where(d > 0, T / d, 0.0), Vk * d
    else:
        genes, cells = Vk, T
    s = rp.sign_rule(genes)
    with np.errstate(divide="ignore", invalid="ignore"):
        res = np.where(th > 0, rho / th, 0.0)
    return {"d": d, "cells": cells * s, "genes": genes * s, "centre": mu, "residuals": res, "converged": int(conv.sum()),
            "cycles": cycles, "products": products, "exhausted": bool(exhausted)}


def dense_svd(M, k: int, centre: bool = False) -> dict:
    """LAPACK on the densified (and centred) matrix, signed by the rule: the yardstick of the yardstick."""
    A = sp.csc_matrix(M).T.toarray()
    if centre:
        A = A - A.mean(axis=0)
    U, d, Vt = np.linalg.svd(A, full_matrices=False)
    kk = min(k, len(d))
    V = Vt.T[:, :kk]
    s = rp.sign_rule(V)
    return {"d": d[:kk], "cells": U[:, :kk] * d[:kk] * s, "genes": V * s, "d_all": d}


def direct_residual(M, r: dict, centre: bool = False):
    """|| A'(A v_i) - d_i^2 v_i || on the host in f64, per component."""
    A = sp.csc_matrix(M).T.toarray()
    if centre:
        A = A - A.mean(axis=0)
    v = r["genes"]
    return np.linalg.norm(A.T @ (A @ v) - v * r["d"] ** 2, axis=0)


def flat(seed: int = 0, G: int = 300, N: int = 500, density: float = 0.1):
    """``sp.random(N, G, density)`` with values in [0.1, 1.1], as the genes x cells CSC matrix: a noise bulk, no separated value
    after the first."""
    rng = np.random.default_rng(seed)
    A = sp.random(N, G, density, random_state=rng, data_rvs=lambda size: rng.uniform(0.1, 1.1, size))
    return sp.csc_matrix(A.T)
