"""NumPy oracle of libgficf_gsea.so (include/gficf_gsea.h): fgsea's calcGseaStat at gseaParam = 0 in its published cumsum form
and in the position form, the hashed permutations, the null table, fgseaSimple's statistics, and the whole call."""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def mix32(x):
    """x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 on uint32 (held in uint64, masked)."""
    x = np.asarray(x, dtype=np.uint64) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    return x ^ (x >> np.uint64(16))


def perm_keys(G, seed, j):
    cj = mix32((np.uint64(int(j) & 0xFFFFFFFF) + mix32(int(seed) & 0xFFFFFFFF)) & _M32)
    return mix32(np.arange(G, dtype=np.uint64) ^ cj)


def perm(G, seed, j):
    """pi_j: the positions [0, G) in ascending order of their hashed keys."""
    return np.argsort(perm_keys(G, seed, j), kind="stable").astype(np.int32)


def order_desc(col):
    """Rows by decreasing statistic, ties (-0.0 == 0.0 among them) by ascending row."""
    return np.argsort(-np.asarray(col, dtype=np.float64), kind="stable")


def ranks(col):
    o = order_desc(col)
    r = np.empty(len(o), dtype=np.int64)
    r[o] = np.arange(len(o))
    return r


def _pick(maxP, minP):
    return maxP if maxP > -minP else (minP if maxP < -minP else 0.0)


def es_literal(stats, rows):
    """fgsea::calcGseaStat(stats, selectedStats, gseaParam = 0, scoreType = "std") as published, on the ordered statistics."""
    stats = np.asarray(stats, dtype=np.float64)
    o = order_desc(stats)
    r = stats[o]
    S = np.sort(ranks(stats)[np.asarray(rows, dtype=np.int64)]) + 1          # selectedStats, sorted
    m, N = len(S), len(r)
    with np.errstate(all="ignore"):
        rAdj = np.abs(r[S - 1]) ** 0                                         # R: 0^0 = 1
    NR = rAdj.sum()
    if NR == 0:
        rCumSum = np.arange(1, m + 1) / m
    else:
        rCumSum = np.cumsum(rAdj) / NR
    tops = rCumSum - (S - np.arange(1, m + 1)) / (N - m)
    bottoms = tops - (1 / m if NR == 0 else rAdj / NR)
    return _pick(tops.max(), bottoms.min())


def es_positions(S, G):
    """The position form: S the ascending 1-based positions of the set among G."""
    S = np.asarray(S, dtype=np.int64)
    m = len(S)
    i = np.arange(1, m + 1, dtype=np.int64)
    top = i.astype(np.float64) / np.float64(m) - (S - i).astype(np.float64) / np.float64(G - m)
    bottom = top - np.float64(1.0) / np.float64(m)
    return _pick(top.max(), bottom.min())


def es_of_set(pos0, G):
    """ES of a set given as 0-based positions in any order."""
    mask = np.zeros(G, dtype=bool)
    mask[np.asarray(pos0, dtype=np.int64)] = True
    return es_positions(np.flatnonzero(mask) + 1, G)


def null(G, seed, sizes, nsim, j0=0):
    """null[d][j]: the ES of {pi_j(0), ..., pi_j(sizes[d] - 1)}."""
    out = np.zeros((len(sizes), nsim), dtype=np.float64)
    for j in range(nsim):
        p = perm(G, seed, j0 + j)
        for d, m in enumerate(sizes):
            out[d, j] = es_of_set(p[:int(m)], G)
    return out


def stats_of(es, x):
    """fgseaSimple's estimator of one set against its null row x: a dict of the four counts, the two means, NES and pval."""
    x = np.asarray(x, dtype=np.float64)
    nGeEs, nLeEs = int((x >= es).sum()), int((x <= es).sum())
    nGeZero, nLeZero = int((x >= 0).sum()), int((x <= 0).sum())
    with np.errstate(all="ignore"):
        geZeroMean = np.float64(np.maximum(x, 0).sum()) / np.float64(nGeZero)
        leZeroMean = np.float64(np.minimum(x, 0).sum()) / np.float64(nLeZero)
        nes = np.float64(es) / (geZeroMean if es > 0 else abs(leZeroMean))
    pval = min(np.float64(1 + nLeEs) / np.float64(1 + nLeZero), np.float64(1 + nGeEs) / np.float64(1 + nGeZero))
    return {"nGeEs": nGeEs, "nLeEs": nLeEs, "nGeZero": nGeZero, "nLeZero": nLeZero, "geZeroMean": geZeroMean, "leZeroMean": leZeroMean,
            "nes": nes, "pval": pval}


def gsea_np(stats, ptr, rows, nsim=1000, min_size=1, max_size=np.inf, seed=180582, null_table=None):
    """The whole call: es, nes, pval, the four counts (P x C), size, tested, sizes, null.  ``null_table``: (sizes, D x nsim)
    computed before, to share it between calls on the same (G, seed, sizes, nsim)."""
    stats = np.asarray(stats, dtype=np.float64)
    if stats.ndim == 1:
        stats = stats[:, None]
    G, C = stats.shape
    ptr = np.asarray(ptr, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int64)
    P = len(ptr) - 1
    size = np.diff(ptr)
    tested = (size >= max(min_size, 1)) & (size <= min(max_size, G - 1))
    sizes = np.unique(size[tested])
    if null_table is not None:
        assert np.array_equal(null_table[0], sizes) and null_table[1].shape == (len(sizes), nsim)
        nu = null_table[1]
    else:
        nu = null(G, seed, sizes, nsim)
    out = {k: np.zeros((P, C), dtype=np.float64) for k in ("es", "nes", "pval")}
    out.update({k: np.zeros((P, C), dtype=np.int64) for k in ("nGeEs", "nLeEs", "nGeZero", "nLeZero")})
    for c in range(C):
        r = ranks(stats[:, c])
        for p in np.flatnonzero(tested):
            es = es_of_set(r[rows[ptr[p]:ptr[p + 1]]], G)
            s = stats_of(es, nu[np.searchsorted(sizes, size[p])])
            out["es"][p, c] = es
            for k in ("nes", "pval", "nGeEs", "nLeEs", "nGeZero", "nLeZero"):
                out[k][p, c] = s[k]
    out.update(size=size, tested=tested, sizes=sizes, null=nu)
    return out
