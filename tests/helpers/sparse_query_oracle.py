"""NumPy oracle of libgficf_sparse_query.so (include/gficf_sparse_query.h) and the comparison rule of its tests.

The oracle is that of the square search (tests/helpers/sparse_knn_oracle.py, unchanged) on the stacked matrix [train | Q]: its
rows N: (the queries) and columns :N (the training cells).  No entry of that block is on the stacked matrix's diagonal, so
nothing of the square search's self rule reaches it.

The rule, for every row of a case: rules 1, 3 and 4 of the square rule (sparse_knn_oracle's docstring), with the ids in [1, N]:
  1. dist ascends, and equal distances have ascending ids;
  3. for every returned id, |q - q_oracle| <= 2^-23 q_oracle + 2^-36 scale;
  4. the row's ids equal the oracle's in order, or differ only in ids whose oracle q is within that tolerance of the oracle's
     k-th q; that second branch is capped at 1 % of a case's rows.
There is no rule 2: a query is no training cell."""
import numpy as np
import scipy.sparse as sp

from tests.helpers import sparse_knn_oracle as so

METRICS = so.METRICS
REL, ABS = so.REL, so.ABS


def cells(G, n, lo, hi, seed, ends=(), hot=0):
    """n cells of ``lo`` .. ``hi`` stored entries each, gamma(2, 1) values at uniformly drawn rows; the cells ``ends`` also store
    the rows 0 and G - 1; with ``hot`` half of a cell's rows come from ``hot`` genes drawn once, so that cells share genes at
    every G."""
    rng = np.random.default_rng(seed)
    hot_genes = rng.choice(G, hot, replace=False) if hot else None
    rows, vals, ptr = [], [], [0]
    for c in range(n):
        m = int(rng.integers(lo, hi + 1))
        r = rng.choice(G, m, replace=False)
        if hot:
            r = np.concatenate([r[:m - m // 2], rng.choice(hot_genes, m // 2, replace=False)])
        if c in ends:
            r = np.concatenate([[0, G - 1], r])
        r = np.unique(r)
        rows.append(r)
        vals.append(rng.gamma(2, 1, len(r)))
        ptr.append(ptr[-1] + len(r))
    return sp.csc_matrix((np.concatenate(vals), np.concatenate(rows).astype(np.int32), np.array(ptr, dtype=np.int32)), shape=(G, n))


# the cases of tests/test_sparse_query_gpu.py that go through the rule: name -> (G, N, M, lo, hi, seed); seeds for which the oracle
# under a permuted summation order takes the rule's second branch in 0 rows (tests/test_sparse_query_cpu.py holds them to that)
BASIC = (300, 150, 37, 12, 40, 7)
BASIC_KS = (1, 16, 64, 65, 128)
SEAM_GS = (4096, 4097, 8192, 8193, 16384, 16385, 32768)
SEAM_N, SEAM_K, SEAM_SEED = 40, 10, 3


def pair_case(G, N, M, lo, hi, seed, ends=(), hot=0):
    """(train, Q) of :func:`cells`, the training cells drawn first."""
    A = cells(G, N + M, lo, hi, seed, ends, hot)
    return sp.csc_matrix(A[:, :N]), sp.csc_matrix(A[:, N:])


def seam_case(G, M):
    """N = 40 training cells of a few entries each and M queries; the first training cell and the last query store the rows 0
    and G - 1."""
    return pair_case(G, SEAM_N, M, 4, 10, SEAM_SEED + G % 97, ends=(0, SEAM_N + M - 1), hot=24)


def permuted(train, Q, seed=1):
    """The same cells with the genes renumbered: the oracle then sums in another order."""
    p = np.random.default_rng(seed).permutation(train.shape[0])
    out = []
    for A in (train, Q):
        A = sp.csc_matrix(A).tocoo()
        B = sp.csc_matrix((A.data, (p[A.row], A.col)), shape=A.shape)
        B.sort_indices()
        out.append(B)
    return out


def stacked(train, Q):
    A = sp.hstack([sp.csc_matrix(train), sp.csc_matrix(Q)], format="csc")
    A.sort_indices()
    return A


def q_and_scale(train, Q, metric):
    """(q, scale): the M x N f64 matrices of rule 3, q before its rounding to f32."""
    N = train.shape[1]
    q, scale = so.q_and_scale(stacked(train, Q), metric)
    return np.ascontiguousarray(q[N:, :N]), np.ascontiguousarray(scale[N:, :N])


def table(q, metric, k):
    """(idx 1-based int32, dist f64 of the f32 value) from q: rounded to f32 once, ordered by (distance, id)."""
    d = (np.sqrt(q) if metric == "euclidean" else q).astype(np.float32)
    order = np.argsort(d, axis=1, kind="stable")[:, :k]                  # stable: equal distances keep ascending ids
    return (order + 1).astype(np.int32), np.take_along_axis(d, order, axis=1).astype(np.float64)


def oracle(train, Q, metric, k):
    q, scale = q_and_scale(train, Q, metric)
    idx, dist = table(q, metric, k)
    return {"idx": idx, "dist": dist, "q": q, "scale": scale}


def brute_force(train, Q, metric, k):
    """The same table by a loop over (query, training cell) pairs and genes, in plain Python floats."""
    A, B = so.dense_cells(Q), so.dense_cells(train)
    G = A.shape[1]
    d = np.zeros((len(A), len(B)), dtype=np.float32)
    for i, a in enumerate(A):
        for j, b in enumerate(B):
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
    M, k = idx.shape
    N = want["q"].shape[1]
    assert want["idx"].shape == (M, k) and dist.shape == (M, k) and idx.dtype == np.int32 and dist.dtype == np.float64
    if M == 0:
        return []
    assert idx.min() >= 1 and idx.max() <= N
    rows = np.arange(M)[:, None]
    # 1
    step_d, step_i = np.diff(dist, axis=1), np.diff(idx, axis=1)
    assert (step_d >= 0).all(), "dist does not ascend"
    assert (step_i[step_d == 0] > 0).all(), "equal distances without ascending ids"
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
    assert len(loose) <= max_loose_share * M, f"{len(loose)} of {M} rows differ from the oracle's ids (near ties at the k-th distance)"
    return loose
