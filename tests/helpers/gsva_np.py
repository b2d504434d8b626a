"""NumPy oracle of libgficf_gsva.so, written from include/gficf_gsva.h the plain way: the dense genes x cells matrix of a
cluster, the all-pairs kernel CDF, ``np.lexsort`` for every cell's order, the sequential random walk, and limma's two-group
contrast by least squares on the design matrix.  The sparse density form and the closed form of the score are here too, so
that tests/test_gsva_cpu.py can hold them against what defines them."""
import numpy as np
from scipy import special, stats

MIN_SD = 1e-10


def phi(v):
    """The standard normal CDF, exactly: 0.5 * erfc(-v / sqrt 2)."""
    return 0.5 * special.erfc(-np.asarray(v, dtype=np.float64) / np.sqrt(2.0))


def gene_filter(X):
    """sd (n - 1) of every row of the dense G x n matrix in two passes, and the kept mask (n >= 2 and sd >= 1e-10)."""
    X = np.asarray(X, dtype=np.float64)
    G, n = X.shape
    if n < 2:
        return np.zeros(G), np.zeros(G, dtype=bool)
    mean = X.sum(axis=1) / n
    sd = np.sqrt(((X - mean[:, None]) ** 2).sum(axis=1) / (n - 1))
    return sd, sd >= MIN_SD


def density_dense(x, sd):
    """d_j of one gene over the n cells of a cluster: L_j = (1 / n) sum_i Phi((x_j - x_i) / bw), bw = sd / 4, i = j included."""
    x = np.asarray(x, dtype=np.float64)
    L = phi((x[:, None] - x[None, :]) / (sd / 4.0)).sum(axis=1) / len(x)
    return -np.log((1.0 - L) / L)


def density_sparse(xnz, n, sd):
    """The same from the stored entries alone (the header's sparse form): (d of every stored entry, d0 of the n - nz zeros)."""
    xnz = np.asarray(xnz, dtype=np.float64)
    bw, z = sd / 4.0, n - len(xnz)
    L = (phi((xnz[:, None] - xnz[None, :]) / bw).sum(axis=1) + z * phi(xnz / bw)) / n
    d0 = 0.0
    if z > 0:
        L0 = (phi(-xnz / bw).sum() + 0.5 * z) / n
        d0 = -np.log((1.0 - L0) / L0)
    return -np.log((1.0 - L) / L), d0


def positions(d):
    """1-based position of every gene in one cell's order: decreasing d, ties by ascending row."""
    d = np.asarray(d, dtype=np.float64)
    o = np.lexsort((np.arange(len(d)), -d))
    pos = np.empty(len(d), dtype=np.int64)
    pos[o] = np.arange(1, len(d) + 1)
    return pos


def rank_scores(Gc):
    """w of the positions 1 .. Gc."""
    S = np.arange(1, Gc + 1, dtype=np.float64)
    return np.abs(Gc - S + 1 - Gc / 2.0)


def es_walk(S, Gc):
    """GSVA's random walk over the positions 1 .. Gc, one step at a time (tau = 1, mx.diff = TRUE, abs.ranking = FALSE): up by
    w / W at a member, down by 1 / (Gc - m) elsewhere; the largest positive excursion plus the largest negative one."""
    inset = np.zeros(Gc, dtype=bool)
    inset[np.asarray(S, dtype=np.int64) - 1] = True
    m = int(inset.sum())
    w = rank_scores(Gc)
    with np.errstate(all="ignore"):
        step = np.where(inset, w / w[inset].sum(), -1.0 / (Gc - m))
    walk = np.cumsum(step)
    if np.isnan(walk).any():
        return np.nan
    return max(0.0, walk.max()) + min(0.0, walk.min())


def es_closed(S, Gc):
    """The header's closed form on the ascending positions S."""
    S = np.sort(np.asarray(S, dtype=np.int64))
    m = len(S)
    w = np.abs((Gc - S + 1).astype(np.float64) - Gc / 2.0)
    W = w.sum()
    if W == 0:
        return np.nan
    i = np.arange(1, m + 1, dtype=np.int64)
    q = (S - i).astype(np.float64) / np.float64(Gc - m)
    cum = np.cumsum(w)
    top = cum / W - q
    bottom = (cum - w) / W - q
    return max(0.0, top.max()) + min(0.0, bottom.min())


def densities(X, cluster, C):
    """Stages 1-2 on the dense G x N matrix: sd, kept (G x C), D (G x N: the density of every (gene, cell), 0 where the gene is
    not kept in the cell's cluster)."""
    X = np.asarray(X, dtype=np.float64)
    G, N = X.shape
    cluster = np.asarray(cluster)
    sd, kept, D = np.zeros((G, C)), np.zeros((G, C), dtype=bool), np.zeros((G, N))
    for c in range(C):
        cells = np.flatnonzero(cluster == c)
        if len(cells) == 0:
            continue
        sd[:, c], kept[:, c] = gene_filter(X[:, cells])
        for g in np.flatnonzero(kept[:, c]):
            D[g, cells] = density_dense(X[g, cells], sd[g, c])
    return sd, kept, D


def scores(D, kept, cluster, C, ptr, members, min_size=1, max_size=np.inf, walk=es_closed):
    """Stages 3-5 from the dense densities: es (P x N), tested (P x C)."""
    G, N = D.shape
    cluster = np.asarray(cluster)
    ptr = np.asarray(ptr, dtype=np.int64)
    members = np.asarray(members, dtype=np.int64)
    P = len(ptr) - 1
    es, tested = np.zeros((P, N)), np.zeros((P, C), dtype=bool)
    for c in range(C):
        cells = np.flatnonzero(cluster == c)
        rows = np.flatnonzero(kept[:, c])
        Gc = len(rows)
        local = np.full(G, -1, dtype=np.int64)
        local[rows] = np.arange(Gc)
        sets = []
        for p in range(P):
            mem = local[members[ptr[p]:ptr[p + 1]]]
            mem = mem[mem >= 0]
            m = len(mem)
            tested[p, c] = len(cells) >= 2 and m >= 1 and max(min_size, 1) <= m <= min(max_size, Gc - 1)
            sets.append(mem)
        if not tested[:, c].any():
            continue
        for j in cells:
            pos = positions(D[rows, j])
            for p in np.flatnonzero(tested[:, c]):
                es[p, j] = walk(pos[sets[p]], Gc)
    return es, tested


def gsva_np(X, cluster, C, ptr, members, min_size=1, max_size=np.inf):
    """The whole call on the dense matrix."""
    sd, kept, D = densities(X, cluster, C)
    es, tested = scores(D, kept, cluster, C, ptr, members, min_size, max_size)
    return {"es": es, "tested": tested, "kept": kept, "sd": sd, "D": D}


def dense_densities(M_csr, cluster, d_nz, d0):
    """The dense G x N density matrix from the library's stage outputs: d_nz where the cell stores the gene, d0 of the cell's
    cluster elsewhere."""
    G, N = M_csr.shape
    D = np.asarray(d0, dtype=np.float64)[:, np.asarray(cluster)].copy()
    rows = np.repeat(np.arange(G), np.diff(M_csr.indptr))
    D[rows, M_csr.indices] = d_nz
    return D


# ------------------------------------------------------------------ limma: lmFit, eBayes, topTable for cluster against the rest
def trigamma_inverse(x):
    if x > 1e7:
        return 1.0 / np.sqrt(x)
    if x < 1e-6:
        return 1.0 / x
    y = 0.5 + 1.0 / x
    for _ in range(50):
        tri = special.polygamma(1, y)
        dif = tri * (1.0 - tri / x) / special.polygamma(2, y)
        y = y + dif
        if -dif / y < 1e-8:
            break
    return float(y)


def fit_f_dist(s2, df1):
    """The prior (s0^2, df0) from the moments of log s^2; df0 = inf when their variance is not positive."""
    x = np.maximum(s2, 0.0)
    m = np.median(x)
    x = np.maximum(x, 1e-5 * (m if m > 0 else 1.0))
    e = np.log(x) - special.digamma(df1 / 2.0) + np.log(df1 / 2.0)
    evar = np.var(e, ddof=1) - special.polygamma(1, df1 / 2.0)
    if evar > 0:
        df0 = 2.0 * trigamma_inverse(float(evar))
        return float(np.exp(e.mean() + special.digamma(df0 / 2.0) - np.log(df0 / 2.0))), df0
    return float(x.mean()), np.inf


def bh(p):
    p = np.asarray(p, dtype=np.float64)
    n = len(p)
    o = np.argsort(p, kind="stable")[::-1]
    q = np.minimum(1.0, np.minimum.accumulate(n / np.arange(n, 0, -1.0) * p[o]))
    out = np.empty(n)
    out[o] = q
    return out


def limma_cluster_vs_rest(Y, in_cluster, cluster_minus_other=False):
    """Y: P' x N scores; the design is model.matrix(~ factor(c("C<label>", "other"))): intercept and the indicator of "other",
    whose coefficient is mean(other) - mean(cluster).  Returns logFC, AveExpr, t, P.Value, adj.P.Val, df0 in the rows' order."""
    Y = np.asarray(Y, dtype=np.float64)
    Pn, N = Y.shape
    X = np.column_stack([np.ones(N), (~np.asarray(in_cluster)).astype(np.float64)])
    XtXi = np.linalg.inv(X.T @ X)
    beta = XtXi @ X.T @ Y.T                                            # 2 x P'
    resid = Y.T - X @ beta
    df = N - 2.0
    s2 = (resid ** 2).sum(axis=0) / df
    if Pn == 1:
        s02, df0 = float(s2[0]), 0.0
    else:
        s02, df0 = fit_f_dist(s2, df)
    post = np.full(Pn, s02) if np.isinf(df0) else (df * s2 + df0 * s02) / (df + df0)
    coef = beta[1]
    t = coef / (np.sqrt(XtXi[1, 1]) * np.sqrt(post))
    dft = min(df + df0, Pn * df)
    pv = 2.0 * stats.t.sf(np.abs(t), dft)
    if cluster_minus_other:
        coef, t = -coef, -t
    return {"logFC": coef, "AveExpr": Y.mean(axis=1), "t": t, "P.Value": pv, "adj.P.Val": bh(pv), "df0": df0}


def de_pathways(es, cluster, C, cluster_minus_other=False):
    """The whole table as arrays: per cluster in id order, the rows of es that are not all zero ordered by decreasing |t|."""
    es = np.asarray(es, dtype=np.float64)
    cluster = np.asarray(cluster)
    use = np.flatnonzero((es != 0).any(axis=1))
    out = {k: [] for k in ("logFC", "AveExpr", "t", "P.Value", "adj.P.Val", "pathway", "cluster")}
    for c in range(C):
        r = limma_cluster_vs_rest(es[use], cluster == c, cluster_minus_other)
        o = np.argsort(-np.abs(r["t"]), kind="stable")
        for k in ("logFC", "AveExpr", "t", "P.Value", "adj.P.Val"):
            out[k].append(r[k][o])
        out["pathway"].append(use[o])
        out["cluster"].append(np.full(len(o), c))
    return {k: np.concatenate(v) for k, v in out.items()}
