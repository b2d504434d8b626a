"""The contract of libgficf_sparse_knn.so (include/gficf_sparse_knn.h) restated in NumPy, rounding for rounding.

Not the kernel's tiling: the header says the result depends on neither the tile of the query nor the slice of the candidate, so
none of that is here.  What is here is the arithmetic, in f64 from the f32-rounded values:

  * a sum over the stored entries e = 0, 1, ... of a column runs in 16 chains, chain l adding the entries l, l + 16, ... in
    order from +0.0 (a column that is no multiple of 16 long is padded with exact zeros, which change nothing), and the
    chains are added in the tree  c = c + c[lane ^ m]  for m = 8, 4, 2, 1 (:func:`chain_sum`);
  * per cell: na = sum a a, la = sum |a|, sa = sum a; the cosine scalar sqrt(na); the correlation mean ma = sa / G and centred
    norm sqrt(na - (G ma) ma), 0 when that difference is not positive (:func:`prepare`);
  * the pair sum of (query, candidate) runs over the CANDIDATE's stored entries against the query's dense values.  The term
    a b of two f32 values is exact in f64, so ``acc + a * b`` is the single rounding of the kernel's fused multiply-add; the
    manhattan term is (|a| + |b|) - |a - b| with every operation rounded as written (a the query's value, b the candidate's);
  * the distance follows ``sk_distance`` operation for operation (the query's scalars first: ``(G ma_query) ma_candidate``),
    ``+ 0.0``, one rounding to f32; the diagonal is 0 without arithmetic;
  * the table is ordered by (f32 distance, id).

``variant`` names a deliberately WRONG order, for tests/test_sparse_knn_par_cpu.py only, which shows that the cases of
tests/helpers/sparse_knn_cases.py tell each from the contract: ``"seq"`` one sequential chain, ``"revtree"`` the tree in the
order ^1, ^2, ^4, ^8, ``"lanes8"`` 8 chains.  ``variant_scope="pair"`` applies it to the pair sums alone (the prepare pass keeps
the contract: a change of the tile kernel only), ``"all"`` to every sum."""
import numpy as np
import scipy.sparse as sp

LANES = 16
METRICS = ("euclidean", "manhattan", "cosine", "correlation")
VARIANTS = ("seq", "revtree", "lanes8")

_ORDERS = {                                                   # variant -> (chains, the tree's masks in order)
    None: (LANES, (8, 4, 2, 1)),
    "seq": (1, ()),
    "revtree": (LANES, (1, 2, 4, 8)),
    "lanes8": (8, (4, 2, 1)),
}


def chain_sum(terms, variant=None):
    """The fixed-order sum of ``terms`` (..., n) f64 along the last axis; returns (...) f64."""
    lanes, masks = _ORDERS[variant]
    t = np.asarray(terms, dtype=np.float64)
    n = t.shape[-1]
    steps = -(-n // lanes)
    if steps * lanes != n:
        t = np.concatenate([t, np.zeros(t.shape[:-1] + (steps * lanes - n,))], axis=-1)
    t = t.reshape(t.shape[:-1] + (steps, lanes))
    c = np.zeros(t.shape[:-2] + (lanes,))
    for s in range(steps):                                    # chain l: entries l, l + lanes, ... in order
        c = c + t[..., s, :]
    lane = np.arange(lanes)
    for m in masks:
        c = c + c[..., lane ^ m]
    return c[..., 0]


def f32_cells(M):
    """(G, N, colptr, rowidx, values as f64 holding the f32-rounded values) of the genes x cells matrix M."""
    M = sp.csc_matrix(M)
    G, N = M.shape
    return G, N, M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data.astype(np.float32).astype(np.float64)


def prepare(M, metric, variant=None):
    """(p0, p1) of ``k_sk_prepare``: p0 = na (euclidean), la (manhattan), sqrt(na) (cosine), the centred norm (correlation);
    p1 = ma (correlation), else 0."""
    G, N, cp, _, x = f32_cells(M)
    na, la, sa = np.zeros(N), np.zeros(N), np.zeros(N)
    for c in range(N):
        a = x[cp[c]:cp[c + 1]]
        na[c], la[c], sa[c] = chain_sum(a * a, variant), chain_sum(np.abs(a), variant), chain_sum(a, variant)
    p1 = np.zeros(N)
    if metric == "euclidean":
        p0 = na
    elif metric == "manhattan":
        p0 = la
    elif metric == "cosine":
        p0 = np.sqrt(na)
    else:
        p1 = sa / float(G)
        v = na - float(G) * p1 * p1                           # (G ma) ma, left to right
        p0 = np.where(v > 0.0, np.sqrt(np.where(v > 0.0, v, 0.0)), 0.0)
    return p0, p1


def _distance(metric, G, S, a0, a1, b0, b1):
    """``sk_distance``: a the query's scalars, b the candidate's; every argument broadcasts."""
    if metric == "euclidean":
        v = (a0 + b0) - 2.0 * S
        return np.sqrt(np.where(v > 0.0, v, 0.0))
    if metric == "manhattan":
        v = (a0 + b0) - S
        return np.where(v > 0.0, v, 0.0)
    num = S - float(G) * a1 * b1 if metric == "correlation" else S
    den = a0 * b0
    zero = (a0 == 0.0) | (b0 == 0.0)
    v = 1.0 - num / np.where(zero, 1.0, den)
    return np.where(zero, 1.0, np.where(v > 0.0, v, 0.0))


def _to_candidate(metric, G, cells, prep, dense, qa0, qa1, c, variant):
    """The f32 distances of the queries (dense values ``dense`` (n_q, G), scalars qa0, qa1) to the candidate c."""
    cp, ri, x = cells
    b, e = cp[c], cp[c + 1]
    av, bv = dense[:, ri[b:e]], x[b:e]                        # over the candidate's stored entries
    terms = (np.abs(av) + np.abs(bv)) - np.abs(av - bv) if metric == "manhattan" else av * bv
    S = chain_sum(terms, variant)
    return (_distance(metric, G, S, qa0, qa1, prep[0][c], prep[1][c]) + 0.0).astype(np.float32)


def _dense(G, cells, queries):
    """The queries' dense values, 0 where nothing is stored."""
    cp, ri, x = cells
    dense = np.zeros((len(queries), G))
    for i, q in enumerate(queries):
        dense[i, ri[cp[q]:cp[q + 1]]] = x[cp[q]:cp[q + 1]]
    return dense


def distance_table(M, metric, q_begin=0, q_end=None, variant=None, variant_scope="all"):
    """The (q_end - q_begin) x N f32 distances of the queries [q_begin, q_end) to every cell."""
    assert metric in METRICS and variant_scope in ("pair", "all")
    G, N, *cells = f32_cells(M)
    q_end = N if q_end is None else q_end
    prep = prepare(M, metric, variant if variant_scope == "all" else None)
    dense = _dense(G, cells, range(q_begin, q_end))
    qa0, qa1 = prep[0][q_begin:q_end], prep[1][q_begin:q_end]
    out = np.empty((q_end - q_begin, N), dtype=np.float32)
    for c in range(N):
        out[:, c] = _to_candidate(metric, G, cells, prep, dense, qa0, qa1, c, variant)
        if q_begin <= c < q_end:
            out[c - q_begin, c] = 0.0                         # the diagonal: no arithmetic
    return out


def pair_distances(M, metric, pairs, variant=None, variant_scope="all"):
    """The mutual f32 distances of the cell pairs (n, 2): (n, 2) f32, [i -> j, j -> i]; the entries of :func:`distance_table`."""
    assert metric in METRICS and variant_scope in ("pair", "all")
    G, N, *cells = f32_cells(M)
    prep = prepare(M, metric, variant if variant_scope == "all" else None)
    out = np.empty((len(pairs), 2), dtype=np.float32)
    for n, (i, j) in enumerate(pairs):
        for side, (q, c) in enumerate(((i, j), (j, i))):
            out[n, side] = _to_candidate(metric, G, cells, prep, _dense(G, cells, [q]), prep[0][q:q + 1], prep[1][q:q + 1], c, variant)[0]
    return out


def table(d, k):
    """(idx 1-based int32, dist f64 of the f32 value), n_q x k, from the f32 distance table: ordered by (distance, id)."""
    assert d.dtype == np.float32 and not np.isnan(d).any()
    order = np.argsort(d, axis=1, kind="stable")[:, :k]      # stable: equal distances keep ascending ids
    return (order + 1).astype(np.int32), np.take_along_axis(d, order, axis=1).astype(np.float64)
