"""numpy f64 port of the randomized SVD of include/gficf_pca.h (Halko / Martinsson / Tropp as rsvd runs it), the yardstick of
tests/test_pca_cpu.py and tests/test_pca_gpu.py, and the planted inputs they use.

The test matrix Omega is an argument.  Two variants of ``orth`` and of the final SVD:
  "lapack"  np.linalg.qr / np.linalg.svd;
  "gram"    the l x l Gram matrix and np.linalg.eigh, as the library does it (orth applied twice; directions with
            lambda <= tau * lambda_max dropped, tau = max(m, 1024) * eps).
The largest deviation between the two on an input is the size of a legitimate difference between two correct f64 evaluations
that orthonormalise differently: ``variant_deviation`` measures it, the GPU tests allow 32 x that (never below 64 eps).
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

EPS = float(np.finfo(np.float64).eps)


def tau(m: int) -> float:
    return max(int(m), 1024) * EPS


def _eigh_desc(S):
    lam, W = np.linalg.eigh(S)
    o = np.argsort(-lam, kind="stable")
    return lam[o], W[:, o]


def orth_lapack(Y):
    return np.linalg.qr(Y)[0]


def orth_gram(Y):
    for _ in range(2):
        lam, W = _eigh_desc(Y.T @ Y)
        keep = (lam > tau(Y.shape[0]) * lam.max()) & (lam > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = np.where(keep, 1.0 / np.sqrt(np.where(keep, lam, 1.0)), 0.0)
        Y = Y @ (W * inv)
    return Y


def sign_rule(genes):
    """+1 / -1 per column: the first entry of largest magnitude becomes positive."""
    i = np.argmax(np.abs(genes), axis=0)
    return np.where(genes[i, np.arange(genes.shape[1])] < 0, -1.0, 1.0)


def rsvd(M_genes_x_cells, omega, k: int, q: int = 2, centre: bool = False, variant: str = "lapack") -> dict:
    """The decomposition of A = t(M) (cells x genes), centred by its column means when asked.  Returns d (k), cells = U d
    (N x k), genes = V (G x k), centre (the gene means or None), d_all (all l values)."""
    orth = {"lapack": orth_lapack, "gram": orth_gram}[variant]
    M = sp.csc_matrix(M_genes_x_cells, dtype=np.float64)
    A = M.T.tocsr()                                           # N x G
    At = M.tocsr()                                            # G x N
    N, G = A.shape
    mu = np.asarray(M.sum(axis=1)).ravel() / N if centre else None

    def to_cells(X):                                          # (A - 1 mu') X
        Y = A @ X
        return Y - (mu @ X)[None, :] if centre else Y

    def to_genes(X):                                          # (A - 1 mu')' X
        Y = At @ X
        return Y - np.outer(mu, X.sum(axis=0)) if centre else Y

    tr = N < G
    to_big, to_small = (to_genes, to_cells) if tr else (to_cells, to_genes)
    omega = np.asarray(omega, dtype=np.float64)
    assert omega.shape[0] == min(N, G)
    Y = to_big(omega)
    for _ in range(q):
        Y = orth(Y)
        Z = orth(to_small(Y))
        Y = to_big(Z)
    Q = orth(Y)
    Z = to_small(Q)                                           # B' (n x l)
    if variant == "lapack":
        W, d, Vt = np.linalg.svd(Z.T, full_matrices=False)
        small, big = Vt.T, Q @ W                              # the vectors on the short and on the tall side
        cells = small * d if tr else big * d
        genes = big if tr else small
    else:
        lam, W = _eigh_desc(Z.T @ Z)
        keep = (lam > tau(Z.shape[0]) * lam.max()) & (lam > 0)
        d = np.where(keep, np.sqrt(np.where(keep, lam, 0.0)), 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = np.where(keep, 1.0 / np.where(keep, d, 1.0), 0.0)
        if tr:
            cells, genes = Z @ (W * keep), Q @ (W * keep)
        else:
            cells, genes = Q @ (W * d), Z @ (W * inv)
    s = sign_rule(genes[:, :k])
    return {"d": d[:k].copy(), "cells": cells[:, :k] * s, "genes": genes[:, :k] * s, "centre": mu, "d_all": d.copy()}


def projector_diff(Q1, Q2) -> float:
    """max |Q1 Q1' - Q2 Q2'|: the two bases span the same range when it vanishes (dense m x m: for the tests' sizes)."""
    return float(np.abs(Q1 @ Q1.T - Q2 @ Q2.T).max())


def align(ref, got):
    """got's columns signed like ref's (by the sign of the column's inner product); for comparisons that must not depend on
    the sign rule."""
    s = np.sign(np.sum(ref * got, axis=0))
    s[s == 0] = 1.0
    return got * s


def deviations(a: dict, b: dict) -> dict:
    """The four figures of the tolerance rule between two results: d relative to d[0], sign-aligned cells / d[0] and genes."""
    d0 = max(a["d"][0], b["d"][0])
    return {"d": float(np.abs(a["d"] - b["d"]).max() / d0),
            "cells": float(np.abs(a["cells"] - align(a["cells"], b["cells"])).max() / d0),
            "genes": float(np.abs(a["genes"] - align(a["genes"], b["genes"])).max())}


def variant_deviation(M, omega, k, q=2, centre=False):
    """(lapack result, gram result, their deviations)."""
    a = rsvd(M, omega, k, q, centre, "lapack")
    b = rsvd(M, omega, k, q, centre, "gram")
    return a, b, deviations(a, b)


def tolerance(dev: float) -> float:
    """The test constant for a measured variant deviation: 32 x, never below 64 eps."""
    return max(32.0 * dev, 64.0 * EPS)


# ---------------------------------------------------------------------------------------------- planted inputs
def blocks(N: int, G: int, cells_per, genes_per, values):
    """C cell groups x disjoint gene sets, constant value a_c in block c, zero elsewhere.  Returns (genes x cells CSC, d, U, V):
    d_c = a_c sqrt(n_c g_c) sorted descending, U (N x C) and V (G x C) the normalised indicators in that order."""
    D = np.zeros((G, N))
    c0 = g0 = 0
    d, U, V = [], [], []
    for n_c, g_c, a in zip(cells_per, genes_per, values):
        D[g0:g0 + g_c, c0:c0 + n_c] = a
        u = np.zeros(N); u[c0:c0 + n_c] = 1 / np.sqrt(n_c)
        v = np.zeros(G); v[g0:g0 + g_c] = 1 / np.sqrt(g_c)
        d.append(a * np.sqrt(n_c * g_c)); U.append(u); V.append(v)
        c0 += n_c; g0 += g_c
    assert c0 <= N and g0 <= G
    o = np.argsort(-np.asarray(d), kind="stable")
    return sp.csc_matrix(D), np.asarray(d)[o], np.stack(U, 1)[:, o], np.stack(V, 1)[:, o]


def planted_sparse(N: int, G: int, C: int, seed: int, noise: float = 0.05, noise_scale: float = 0.25):
    """Group programmes scaled by 0.8^c plus sparse noise: group c owns N / C cells and G / (2 C) genes, its block holds
    0.8^c * a_i * b_j with a, b uniform in [0.5, 1.5] and scaled to the norms sqrt(N / C), sqrt(G / (2 C)), so that the
    programmes' values are 0.8^c sqrt(N G / 2) / C: 20 % apart before the noise; `noise` of all entries carry N(0, s) with s
    chosen so that the noise's largest singular value is about `noise_scale` of the weakest programme's.  Genes x cells CSC."""
    rng = np.random.default_rng(seed)
    nc, gc = N // C, G // (2 * C)
    D = np.zeros((G, N))
    weakest = 0.0
    for c in range(C):
        a, b = rng.uniform(0.5, 1.5, nc), rng.uniform(0.5, 1.5, gc)
        a, b = a * (np.sqrt(nc) / np.linalg.norm(a)), b * (np.sqrt(gc) / np.linalg.norm(b))
        D[c * gc:(c + 1) * gc, c * nc:(c + 1) * nc] = 0.8 ** c * np.outer(b, a)
        weakest = 0.8 ** c * np.linalg.norm(a) * np.linalg.norm(b)
    s = noise_scale * weakest / (np.sqrt(noise * N) + np.sqrt(noise * G))
    mask = rng.random((G, N)) < noise
    D = D + mask * rng.standard_normal((G, N)) * s
    return sp.csc_matrix(D)


def assert_separated(d_all, k: int, by: float = 0.10):
    """Every one of the k leading values differs from its neighbours by at least `by` of itself."""
    d = np.asarray(d_all, dtype=np.float64)
    assert len(d) > k, "the sketch must hold the value after the k-th"
    for i in range(k):
        assert d[i] - d[i + 1] >= by * d[i], (i, d[:k + 1])


def planted_counts(N: int, C: int, G: int, seed: int, prog: int = 40, high: float = 6.0, low: float = 0.3):
    """Count matrix (genes x cells CSC, float64) of C cell groups with disjoint gene programmes: group c's `prog` genes are
    Poisson(high) in its cells and Poisson(low / 10) elsewhere, the remaining genes Poisson(low) everywhere.  Returns
    (M, group of every cell)."""
    rng = np.random.default_rng(seed)
    group = np.arange(N) % C
    lam = np.full((G, N), low)
    for c in range(C):
        lam[c * prog:(c + 1) * prog, :] = low / 10
        lam[c * prog:(c + 1) * prog, group == c] = high
    return sp.csc_matrix(rng.poisson(lam).astype(np.float64)), group
