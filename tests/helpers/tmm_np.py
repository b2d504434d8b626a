"""Dense NumPy port of include/gficf_tmm.h, written the plain way from the header: the yardstick of tests/test_tmm_gpu.py.

Two rank modes: ``keys="canonical"`` ranks on q = obs / ref and s = obs * ref (the contract); ``keys="literal"`` ranks
logR and absE as computed, with scipy.stats.rankdata: edgeR as written.  Sums are NumPy's (pairwise), not the library's folded
ones: they differ by summation order only."""
import math

import numpy as np


def col_stats(X):
    """lib, sq, f75, the two order statistics (2 x N) and G' of the dense genes x cells matrix X."""
    X = np.asarray(X, dtype=np.float64)
    Xk = X[(X > 0).any(axis=1)]                                           # calcNormFactors drops the all-zero rows
    Gp, N = Xk.shape
    lib, sq = X.sum(axis=0), np.sqrt(X).sum(axis=0)
    if Gp == 0:
        return lib, sq, np.zeros(N), np.zeros((2, N)), 0
    idx = (Gp - 1) * 0.75
    lo, hi = math.floor(idx), math.ceil(idx)
    S = np.sort(Xk, axis=0)
    xlo, xhi = S[lo].copy(), S[hi].copy()
    q, h = xlo.copy(), idx - lo
    m = (idx > lo) & (xhi != q)
    q[m] = (1 - h) * q[m] + h * xhi[m]
    with np.errstate(invalid="ignore", divide="ignore"):
        f75 = np.where(lib > 0, q / lib, 0.0)
    return lib, sq, f75, np.stack([xlo, xhi]), Gp


def choose_ref(f75, sq):
    """edgeR's reference column and the relative margin of the extremum over the runner-up."""
    f75, sq = np.asarray(f75), np.asarray(sq)
    if np.median(f75) < 1e-20:
        o = np.argsort(-sq, kind="stable")
        return int(o[0]), float((sq[o[0]] - sq[o[1]]) / sq[o[0]]) if len(o) > 1 else 1.0
    d = np.abs(f75 - math.fsum(f75) / len(f75))
    o = np.argsort(d, kind="stable")
    return int(o[0]), float((d[o[1]] - d[o[0]]) / d[o[1]]) if len(o) > 1 else 1.0


def avg_rank(v):
    """#less + (#equal + 1) / 2 of every element of v."""
    s = np.sort(v)
    less, leq = np.searchsorted(s, v, "left"), np.searchsorted(s, v, "right")
    return less + (leq - less + 1) / 2.0


def cell_factor(obs, ref, nO, nR, logratioTrim=.3, sumTrim=.05, doWeighting=True, keys="canonical"):
    """(factor, n, kept, keep mask over the common entries) of one cell against the reference column."""
    m = (obs > 0) & (ref > 0)
    o, r = obs[m], ref[m]
    n = len(o)
    if n == 0:
        return 1.0, 0, 0, np.zeros(0, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        logR = np.log2((o / nO) / (r / nR))
        absE = (np.log2(o / nO) + np.log2(r / nR)) / 2
        v = (nO - o) / nO / o + (nR - r) / nR / r
        if keys == "canonical":
            rq, rs = avg_rank(o / r), avg_rank(o * r)
        else:
            from scipy.stats import rankdata

            rq, rs = rankdata(logR), rankdata(absE)
        loL = math.floor(n * logratioTrim) + 1
        hiL = n + 1 - loL
        loS = math.floor(n * sumTrim) + 1
        hiS = n + 1 - loS
        keep = (rq >= loL) & (rq <= hiL) & (rs >= loS) & (rs <= hiS)
        if doWeighting:
            a, b = logR[keep] / v[keep], 1 / v[keep]
            f = a[~np.isnan(a)].sum() / b[~np.isnan(b)].sum()
        else:
            a = logR[keep]
            a = a[~np.isnan(a)]
            f = a.sum() / len(a) if len(a) else np.nan
        fac = float(np.exp2(f))
    if np.isnan(f) or np.abs(logR).max() < 1e-6:
        fac = 1.0
    return fac, n, int(keep.sum()), keep


def calc_norm_factors(X, refColumn=None, logratioTrim=.3, sumTrim=.05, doWeighting=True, keys="canonical"):
    X = np.asarray(X, dtype=np.float64)
    N = X.shape[1]
    lib, sq, f75, ostat, Gp = col_stats(X)
    ref = choose_ref(f75, sq)[0] if refColumn is None else int(refColumn)
    raw, n, kept = np.ones(N), np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    for c in range(N):
        raw[c], n[c], kept[c], _ = cell_factor(X[:, c], X[:, ref], lib[c], lib[ref], logratioTrim, sumTrim, doWeighting, keys)
    f = raw / np.exp(np.mean(np.log(raw)))
    return {"norm.factors": f, "lib.size": lib, "refColumn": ref, "f75": f75, "n": n, "kept": kept, "sq": sq, "ostat": ostat, "Gprime": Gp,
            "factors.raw": raw}


def cpm(X, lib, f):
    """x / (1e-6 * (lib * f)), the three operations of the header."""
    return np.asarray(X, dtype=np.float64) / (1e-6 * (np.asarray(lib) * np.asarray(f)))[None, :]


# ------------------------------------------------------------------ the inputs the CPU and the GPU tests share
EDGE_N = (0, 1, 2, 3, 4, 9, 10, 11, 19, 20, 21, 59, 60, 61, 63, 64, 65, 500)   # trim-index boundaries, the capacity 64 and a long cell


def gamma_poisson(G=3000, N=200, seed=3):
    """Dense-ish counts (most cells hold more than a quarter of the genes): the f75 branch of the reference choice."""
    rng = np.random.default_rng(seed)
    mu = rng.lognormal(0.0, 1.2, G)[:, None] * rng.lognormal(0.0, 0.3, N)[None, :]
    return rng.poisson(rng.gamma(2.0, mu / 2.0)).astype(np.float64)


def edge_matrix(seed=11):
    """800 genes: column 0 (the reference) holds rows 0..599; then one cell per n of EDGE_N with n rows of the reference's and a
    few of rows 600..779; a copy of the reference; a cell with a single gene; an empty column.  Rows 780..799 are all zero and
    row 779 holds a stored zero only.  Returns (dense X, scipy CSC with the stored zero)."""
    import scipy.sparse as sp

    rng = np.random.default_rng(seed)
    G = 800
    cols = [np.zeros(G)]
    cols[0][:600] = rng.integers(1, 40, 600)
    for n in EDGE_N:
        c = np.zeros(G)
        c[rng.permutation(600)[:n]] = rng.integers(1, 12, n)
        extra = rng.integers(3, 40)
        c[600 + rng.permutation(179)[:extra]] = rng.integers(1, 12, extra)
        cols.append(c)
    cols.append(cols[0].copy())
    single = np.zeros(G)
    single[17] = 5.0
    cols += [single, np.zeros(G)]
    X = np.stack(cols, axis=1)
    M = sp.csc_matrix(X)
    M.sort_indices()
    # a stored zero: row 779 of column 1, appended behind its other rows
    ptr, idx, dat = M.indptr.astype(np.int64), M.indices, M.data
    at = ptr[2]
    idx, dat = np.insert(idx, at, 779), np.insert(dat, at, 0.0)
    ptr[2:] += 1
    Mz = sp.csc_matrix((dat, idx, ptr), shape=X.shape)
    Mz.has_sorted_indices = True
    return X, Mz


def multiples_matrix(G=300, N=12, seed=5):
    """Every column an integer multiple of column 0: every logR is 0."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 30, G).astype(np.float64) * (rng.random(G) < .6)
    k = np.concatenate([[1], rng.integers(1, 9, N - 1)]).astype(np.float64)
    return base[:, None] * k[None, :]


def boosted_matrix(G=400, N=6, seed=9):
    """Column 0 the reference; every other column equals it except that fewer than 30 % of its genes, none of the top tenth by
    count, are multiplied by 8.  Returns (X, the mask of the changed entries)."""
    rng = np.random.default_rng(seed)
    base = rng.integers(1, 200, G).astype(np.float64)
    low = np.flatnonzero(base <= np.quantile(base, .9))
    X = np.repeat(base[:, None], N, axis=1)
    changed = np.zeros((G, N), dtype=bool)
    for c in range(1, N):
        pick = rng.permutation(low)[:int(G * .05 * c)]       # 5 % .. 25 % of the genes
        changed[pick, c] = True
    X[changed] *= 8
    return X, changed


# ------------------------------------------------------------------ derived answers, no oracle in the loop
def check_multiples(X, res, cpms):
    """Every column an integer multiple of the reference: logR = 0 everywhere, every factor exactly 1, cpm = plain CPM."""
    assert np.array_equal(res["norm.factors"], np.ones(X.shape[1])) and np.array_equal(res["lib.size"], X.sum(axis=0))
    assert np.array_equal(res["n"], np.full(X.shape[1], (X[:, 0] > 0).sum()))
    assert np.array_equal(cpms, X / (1e-6 * X.sum(axis=0))[None, :])


def check_boosted(X, changed, res, cpms):
    """The boosted genes are trimmed: f * nO = nR, and the untouched genes have the reference column's CPMs."""
    ref = res["refColumn"]
    assert ref == 0
    eff = res["norm.factors"] * res["lib.size"]
    np.testing.assert_allclose(eff, eff[0], rtol=1e-12)
    assert (res["kept"] <= res["n"] - changed.sum(axis=0)).all() and (res["n"] == X.shape[0]).all()
    for c in range(1, X.shape[1]):
        u = ~changed[:, c]
        np.testing.assert_allclose(cpms[u, c], cpms[u, 0], rtol=1e-12)
