"""NumPy oracle of the marker-gene test (findClusterMarkers, reference R/deGenes.R:15-60; the per-row test of
src/rcpp_parallel_mann_whitney.cpp with the helpers of src/mann_whitney.cpp), written from the stated semantics:

  ranks     average ranks over all N values of the gene, ties by exact f64 equality (-0.0 == 0.0)
  U1, U2    R_1 - n1(n1+1)/2, R_2 - n2(n2+1)/2 (exact: half-integers)
  mu        floor(n1 n2 / 2)
  z         (U1 < U2 ? U1 - mu : U2 - mu), then +0.5 if < 0 else -0.5, then / sigma
  sigma     sqrt((n1 n2 / 12) ((n1 + n2 + 1) - T / ((n1 + n2)(n1 + n2 - 1)))), T = sum of t^3 - t over the tie groups
  p         erfc(|z| / sqrt(2)); 1 when the gene holds a single distinct value
  log2FC    log2(avg(v1 + 1) / avg(v2 + 1))

Two forms: ``wmu_literal`` concatenates, sorts and ranks for every (gene, split) as the reference does; ``markers_shared`` ranks
every gene once and takes the per-cluster rank sums from it (the one-sort-per-gene idea, dense rows, no sparsity tricks);
``markers_sparse`` does the same for all genes at once from the stored non-zeros.
"""
from __future__ import annotations

import math

import numpy as np


def _sigma(n1: int, n2: int, T) -> float:
    d1, d2 = float(n1), float(n2)
    return math.sqrt((d1 * d2 / 12) * ((d1 + d2 + 1) - float(T) / ((d1 + d2) * (d1 + d2 - 1))))


def _z_p(U1: float, U2: float, n1: int, n2: int, T, ndistinct: int):
    if ndistinct <= 1:
        return float("nan"), 1.0
    mu = (n1 * n2) // 2
    z = (U1 - mu) if U1 < U2 else (U2 - mu)
    z = z + 0.5 if z < 0 else z - 0.5
    z = z / _sigma(n1, n2, T)
    return z, math.erfc(abs(z) / math.sqrt(2.0))


def _avg_ranks(sorted_vals: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """getRanks / getCounts of the reference on ascending values: (average 1-based ranks, tie-group sizes)."""
    n = len(sorted_vals)
    head = np.ones(n, dtype=bool)
    head[1:] = sorted_vals[1:] != sorted_vals[:-1]
    starts = np.flatnonzero(head)
    sizes = np.diff(np.append(starts, n))
    ranks = np.repeat(1 + (2 * starts + sizes - 1) / 2.0, sizes)
    return ranks, sizes


def wmu_literal(v1, v2) -> dict:
    """One test as the reference runs it: concatenate, sort, rank, sum.  Returns U1, U2, T, z, p, lfc."""
    v1 = np.asarray(v1, dtype=np.float64)
    v2 = np.asarray(v2, dtype=np.float64)
    n1, n2 = len(v1), len(v2)
    values = np.concatenate([v1, v2])
    idx = np.argsort(values, kind="stable")
    ranks, sizes = _avg_ranks(values[idx])
    U1 = -0.5 * n1 * (n1 + 1) + float(ranks[idx < n1].sum())
    U2 = -0.5 * n2 * (n2 + 1) + float(ranks[idx >= n1].sum())
    T = 0.0
    for t in sizes:                                        # the reference's running f64 sum, in group order
        T += float(t) ** 3 - float(t)
    z, p = _z_p(U1, U2, n1, n2, T, len(sizes))
    s1 = 0.0
    for v in v1:
        s1 += v + 1.0
    s2 = 0.0
    for v in v2:
        s2 += v + 1.0
    return {"U1": U1, "U2": U2, "T": int(T), "z": z, "p": p, "lfc": math.log2((s1 / n1) / (s2 / n2))}


def wmu_dense_literal(X, Y) -> np.ndarray:
    """rcpp_parallel_WMU_test(X, Y) by ``wmu_literal`` row by row: G x 2 [p, log2FC]."""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    out = np.empty((X.shape[0], 2))
    for g in range(X.shape[0]):
        r = wmu_literal(X[g], Y[g])
        out[g] = r["p"], r["lfc"]
    return out


def markers_literal(M, ids, C: int) -> dict:
    """Every (gene, cluster) by ``wmu_literal`` on the dense genes x cells matrix M: G x C arrays U1, U2, T, z, p, lfc."""
    M = np.asarray(M, dtype=np.float64)
    ids = np.asarray(ids)
    G = M.shape[0]
    out = {k: np.empty((G, C)) for k in ("U1", "U2", "z", "p", "lfc")}
    out["T"] = np.empty((G, C), dtype=np.int64)
    for c in range(C):
        inn, rest = ids == c, ids != c
        for g in range(G):
            r = wmu_literal(M[g, inn], M[g, rest])
            for k in out:
                out[k][g, c] = r[k]
    return out


def markers_shared(M, ids, C: int) -> dict:
    """The same by one sort per gene: ranks of the full row, rank sums per cluster by bincount.  M: dense or scipy sparse."""
    import scipy.sparse as sp

    ids = np.asarray(ids, dtype=np.int64)
    R = sp.csr_matrix(M) if sp.issparse(M) else None
    G, N = M.shape
    n1 = np.bincount(ids, minlength=C).astype(np.int64)
    n2 = N - n1
    out = {k: np.empty((G, C)) for k in ("U1", "U2", "z", "p", "lfc")}
    out["T"] = np.empty((G, C), dtype=np.int64)
    for g in range(G):
        row = R[g].toarray().ravel() if R is not None else np.asarray(M[g], dtype=np.float64)
        row = row + 0.0                                    # -0.0 -> 0.0 (equal anyway under ==)
        idx = np.argsort(row, kind="stable")
        ranks_sorted, sizes = _avg_ranks(row[idx])
        r2 = np.empty(N, dtype=np.int64)
        r2[idx] = np.rint(2 * ranks_sorted).astype(np.int64)
        R2c = np.bincount(ids, weights=r2, minlength=C).astype(np.int64)        # exact below 2^53
        R2r = N * (N + 1) - R2c
        T = int((sizes.astype(np.int64) ** 3 - sizes).sum())
        Sc = np.bincount(ids, weights=row, minlength=C)
        Sr = row.sum() - Sc
        for c in range(C):
            U1 = (R2c[c] - n1[c] * (n1[c] + 1)) / 2.0
            U2 = (R2r[c] - n2[c] * (n2[c] + 1)) / 2.0
            z, p = _z_p(U1, U2, int(n1[c]), int(n2[c]), T, len(sizes))
            out["U1"][g, c], out["U2"][g, c], out["T"][g, c], out["z"][g, c], out["p"][g, c] = U1, U2, T, z, p
        out["lfc"][g] = np.log2(((Sc + n1) / n1) / ((Sr + n2) / n2))
    return out


def markers_sparse(M, ids, C: int) -> dict:
    """The same, vectorised over all genes (10^6 genes, 10^7 non-zeros): one lexsort of the stored non-zeros by (gene, value),
    the zeros counted rather than stored (one tie group between the negatives and the positives).  2 x rank sums by bincount
    over gene * C + cluster (exact below 2^53), T in int64, z and p in the expression order of ``_z_p`` (p bit for bit).
    lfc: per-cluster f64 sums, the rest's as the sum over the clusters before it plus the sum over those after it (no
    total - cluster cancellation).  M: scipy sparse or dense, genes x cells."""
    import scipy.sparse as sp

    ids = np.asarray(ids, dtype=np.int64)
    coo = sp.coo_matrix(M)
    G, N = coo.shape
    v = coo.data.astype(np.float64) + 0.0                  # -0.0 -> 0.0
    nz = v != 0.0
    gene, cell, v = coo.row[nz].astype(np.int64), coo.col[nz].astype(np.int64), v[nz]
    o = np.lexsort((v, gene))
    gene, cell, v = gene[o], cell[o], v[o]
    cl = ids[cell]
    nnz = len(v)
    n1 = np.bincount(ids, minlength=C).astype(np.int64)
    n2 = N - n1
    neg = np.bincount(gene[v < 0], minlength=G).astype(np.int64)
    pos = np.bincount(gene[v > 0], minlength=G).astype(np.int64)
    Z = N - neg - pos
    gstart = np.searchsorted(gene, np.arange(G))           # first sorted position of every gene
    head = np.ones(nnz, dtype=bool)
    head[1:] = (gene[1:] != gene[:-1]) | (v[1:] != v[:-1])
    starts = np.flatnonzero(head)
    sizes = np.diff(np.append(starts, nnz)).astype(np.int64)
    grp = np.cumsum(head) - 1
    s, t = starts[grp], sizes[grp]
    pos0 = s - gstart[gene] + np.where(v > 0, Z[gene], 0)  # 0-based place of the group among all N values of the gene
    r2 = 2 * pos0 + t + 1                                   # 2 x average 1-based rank
    lin = gene * C + cl
    R2c = np.bincount(lin, weights=r2, minlength=G * C).astype(np.int64).reshape(G, C)
    cnt = np.bincount(lin, minlength=G * C).astype(np.int64).reshape(G, C)
    R2c += (n1[None, :] - cnt) * (2 * neg + Z + 1)[:, None]
    R2r = N * (N + 1) - R2c
    T = np.zeros(G, dtype=np.int64)
    np.add.at(T, gene[starts], sizes ** 3 - sizes)
    T += Z ** 3 - Z
    ndist = np.bincount(gene[starts], minlength=G) + (Z > 0)
    n1b, n2b = np.broadcast_to(n1, (G, C)), np.broadcast_to(n2, (G, C))
    U1 = (R2c - n1b * (n1b + 1)) / 2.0
    U2 = (R2r - n2b * (n2b + 1)) / 2.0
    mu = (n1b * n2b) // 2
    z = np.where(U1 < U2, U1 - mu, U2 - mu)
    z = np.where(z < 0, z + 0.5, z - 0.5)
    d1, d2 = n1b.astype(np.float64), n2b.astype(np.float64)
    Tf = np.broadcast_to(T.astype(np.float64)[:, None], (G, C))
    with np.errstate(invalid="ignore", divide="ignore"):   # (sigma = 0 only where a gene holds one value: p = 1 there)
        z = z / np.sqrt((d1 * d2 / 12) * ((d1 + d2 + 1) - Tf / ((d1 + d2) * (d1 + d2 - 1))))
    one = np.broadcast_to((ndist <= 1)[:, None], (G, C))
    z = np.where(one, np.nan, z)
    p = np.frompyfunc(math.erfc, 1, 1)(np.abs(z) / math.sqrt(2.0)).astype(np.float64)
    p[one] = 1.0
    Sc = np.bincount(lin, weights=v, minlength=G * C).reshape(G, C)
    before = np.cumsum(np.concatenate([np.zeros((G, 1)), Sc[:, :-1]], axis=1), axis=1)
    after = np.cumsum(np.concatenate([np.zeros((G, 1)), Sc[:, :0:-1]], axis=1), axis=1)[:, ::-1]
    Sr = before + after
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        lfc = np.log2(((Sc + n1b) / n1b) / ((Sr + n2b) / n2b))
    return {"U1": U1, "U2": U2, "T": np.broadcast_to(T[:, None], (G, C)).copy(), "z": z, "p": p, "lfc": lfc}


def p_adjust_bh(p) -> np.ndarray:
    """p.adjust(p, "fdr") written out as a loop: q_(i) = min over j >= i of n p_(j) / j (ascending p), capped at 1."""
    p = np.asarray(p, dtype=np.float64)
    n = len(p)
    o = np.argsort(p, kind="stable")
    q = np.empty(n)
    run = 1.0
    for k in range(n - 1, -1, -1):
        run = min(run, n / (k + 1) * p[o[k]])
        q[o[k]] = run
    return q


def find_cluster_markers(P, LFC, labels, names) -> list[tuple]:
    """R's post-processing of findClusterMarkers (R/deGenes.R:48-57) on G x C p-values and fold changes: rows
    (ens, log2FC, p.value, fdr, cluster) in the reference's order."""
    rows = []
    for j, lab in enumerate(labels):
        fdr = p_adjust_bh(P[:, j])
        sel = [g for g in range(P.shape[0]) if fdr[g] < .05 and LFC[g, j] > 0]
        sel.sort(key=lambda g: fdr[g])                     # stable
        rows += [(names[g], LFC[g, j], P[g, j], fdr[g], lab) for g in sel]
    rows.sort(key=lambda r: -r[1])                         # stable, decreasing log2FC
    return rows
