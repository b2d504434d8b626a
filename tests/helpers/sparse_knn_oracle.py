"""NumPy oracle of libgficf_sparse_knn.so (include/gficf_sparse_knn.h) and the comparison rule of its tests.

The oracle: the values rounded to f32, the header's formulas in f64 on the DENSIFIED matrix (cosine and correlation clamped at 0
from below, as the header states), the diagonal set to 0, one rounding to f32, the table ordered by (distance, id).  Its
summation order is numpy's, not the kernel's: the comparison rule allows for that and for nothing else.

The rule, for every row of a case:
  1. dist ascends, and equal distances have ascending ids;
  2. dist[:, 0] == 0, and cell i is in its own row;
  3. for every returned id, |q - q_oracle| <= 2^-23 q_oracle + 2^-36 scale, q = d^2 (euclidean) or d, scale = na + nb
     (euclidean), la + lb (manhattan), 1 (cosine, correlation): one f32 rounding, plus the worst-case f64 summation bound
     n 2^-53 at n <= 2^15 terms with a factor 4 for the operations after the sum;
  4. the row's ids equal the oracle's in order, or differ only in ids whose oracle q is within that tolerance of the oracle's
     k-th q; that second branch is capped at 1 % of a case's rows (measured on the CPU under a permuted summation order: 0)."""
import numpy as np
import scipy.sparse as sp

METRICS = ("euclidean", "manhattan", "cosine", "correlation")
REL, ABS = 2.0 ** -23, 2.0 ** -36


def case(G, N, density, seed):
    """The data of every oracle case: gamma(2, 1) values at uniformly drawn places, genes x cells CSC."""
    rng = np.random.default_rng(seed)
    M = sp.random(G, N, density, random_state=rng, data_rvs=lambda n: rng.gamma(2, 1, n), format="csc")
    M.sort_indices()
    return M


def dense_cells(M):
    """The cells as rows, N x G f64 holding the f32-rounded values."""
    return np.asarray(sp.csc_matrix(M).astype(np.float32).T.todense(), dtype=np.float64)


def q_and_scale(M, metric):
    """(q, scale): the N x N f64 matrices of rule 3, q before its rounding to f32, the diagonal 0."""
    A = dense_cells(M)
    N, G = A.shape
    na = (A * A).sum(axis=1)
    if metric == "manhattan":
        la = np.abs(A).sum(axis=1)
        q = np.empty((N, N))
        for i in range(N):
            T = ((np.abs(A[i]) + np.abs(A)) - np.abs(A[i] - A)).sum(axis=1)
            q[i] = np.maximum(0.0, (la[i] + la) - T)
        scale = la[:, None] + la[None, :]
    else:
        S = A @ A.T
        if metric == "euclidean":
            q = np.maximum(0.0, (na[:, None] + na[None, :]) - 2.0 * S)
            scale = na[:, None] + na[None, :]
        else:
            if metric == "correlation":
                ma = A.sum(axis=1) / G
                v = na - G * ma * ma
                r = np.sqrt(np.maximum(v, 0.0))
                S = S - G * ma[:, None] * ma[None, :]
            else:
                r = np.sqrt(na)
            rr = r[:, None] * r[None, :]
            with np.errstate(divide="ignore", invalid="ignore"):
                q = np.where(rr == 0.0, 1.0, np.maximum(0.0, 1.0 - S / rr))
            scale = np.ones((N, N))
    np.fill_diagonal(q, 0.0)
    return q, scale


def table(q, metric, k):
    """(idx 1-based int32, dist f64 of the f32 value) from q: rounded to f32 once, ordered by (distance, id)."""
    d = (np.sqrt(q) if metric == "euclidean" else q).astype(np.float32)
    np.fill_diagonal(d, 0.0)
    order = np.argsort(d, axis=1, kind="stable")[:, :k]                  # stable: equal distances keep ascending ids
    return (order + 1).astype(np.int32), np.take_along_axis(d, order, axis=1).astype(np.float64)


def oracle(M, metric, k):
    q, scale = q_and_scale(M, metric)
    idx, dist = table(q, metric, k)
    return {"idx": idx, "dist": dist, "q": q, "scale": scale}


def brute_force(M, metric, k):
    """The same table by a loop over pairs and genes, in plain Python floats (for the oracle's own test)."""
    A = dense_cells(M)
    N, G = A.shape
    d = np.zeros((N, N), dtype=np.float32)
    for i in range(N):
        for j in range(N):
            if i == j:
                continue
            a, b = A[i], A[j]
            S = sum(float(x) * float(y) for x, y in zip(a, b))
            na, nb = sum(float(x) ** 2 for x in a), sum(float(y) ** 2 for y in b)
            if metric == "euclidean":
                v = float(np.sqrt(max(0.0, na + nb - 2.0 * S)))
            elif metric == "manhattan":
                v = max(0.0, sum(abs(float(x)) for x in a) + sum(abs(float(y)) for y in b)
                        - sum(abs(float(x)) + abs(float(y)) - abs(float(x) - float(y)) for x, y in zip(a, b)))
            else:
                if metric == "correlation":
                    ma, mb = sum(map(float, a)) / G, sum(map(float, b)) / G
                    S, na, nb = S - G * ma * mb, na - G * ma * ma, nb - G * mb * mb
                ra, rb = float(np.sqrt(max(na, 0.0))), float(np.sqrt(max(nb, 0.0)))
                v = 1.0 if ra == 0.0 or rb == 0.0 else max(0.0, 1.0 - S / (ra * rb))
            d[i, j] = v
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    return (order + 1).astype(np.int32), np.take_along_axis(d, order, axis=1).astype(np.float64)


def compare(got, want, metric, abs_term=ABS, max_loose_share=0.01):
    """The comparison rule on every row; ``want``: :func:`oracle`'s dict.  Returns the rows that took the second branch of rule 4."""
    idx, dist = np.asarray(got["idx"]), np.asarray(got["dist"])
    N, k = idx.shape
    assert want["idx"].shape == (N, k) and dist.shape == (N, k) and idx.dtype == np.int32 and dist.dtype == np.float64
    assert idx.min() >= 1 and idx.max() <= N
    rows = np.arange(N)[:, None]
    # 1
    step_d, step_i = np.diff(dist, axis=1), np.diff(idx, axis=1)
    assert (step_d >= 0).all(), "dist does not ascend"
    assert (step_i[step_d == 0] > 0).all(), "equal distances without ascending ids"
    # 2
    assert (dist[:, 0] == 0).all() and (idx == rows + 1).any(axis=1).all(), "a cell is not in its own row at distance 0"
    # 3
    q = dist * dist if metric == "euclidean" else dist
    qo, sc = want["q"][rows, idx - 1], want["scale"][rows, idx - 1]
    err, tol = np.abs(q - qo), REL * qo + abs_term * sc
    worst = np.unravel_index(np.argmax(err - tol), err.shape)
    assert (err <= tol).all(), f"row {worst[0]} id {idx[worst]}: q = {q[worst]!r}, oracle {qo[worst]!r}, tolerance {tol[worst]:.3e}"
    # 4
    loose = []
    for i in np.flatnonzero((idx != want["idx"]).any(axis=1)):
        differ = idx[i] != want["idx"][i]
        ids = np.union1d(idx[i][differ], want["idx"][i][differ]) - 1
        kth = want["q"][i, want["idx"][i, k - 1] - 1]
        qi, si = want["q"][i, ids], want["scale"][i, ids]
        assert (np.abs(qi - kth) <= REL * kth + abs_term * si).all(), f"row {i}: ids {ids + 1} differ from the oracle's away from its k-th distance"
        loose.append(int(i))
    assert len(loose) <= max_loose_share * N, f"{len(loose)} of {N} rows differ from the oracle's ids (near ties at the k-th distance)"
    return loose
