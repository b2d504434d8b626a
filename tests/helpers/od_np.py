"""The oracle of libgficf_od.so, written from the contract of include/gficf_od.h (not from the kernels): NumPy / SciPy for the
spline (explicit X and S, the same fixed search for lambda, the fit by a dense solve of the augmented least-squares problem),
mpmath at 50 digits for the two special functions (series of positive terms and a continued fraction evaluated from its tail,
the quantile by bracketed root finding), ``bh.adjust`` and the selection rule literally."""
import functools
import math

import mpmath as mp
import numpy as np

mp.mp.dps = 50
LN10 = math.log(10.0)
RHO_GRID = [LN10 * (-12.0 + j / 4.0) for j in range(97)]


# ------------------------------------------------------------------ the spline
def place_knots(x, k):
    """mgcv's place.knots on the distinct values of x: None where there are fewer than k."""
    u = np.unique(np.asarray(x, dtype=np.float64))
    if len(u) < k:
        return None
    t = np.arange(k) * (len(u) - 1) / (k - 1)
    lo, hi = np.floor(t).astype(int), np.ceil(t).astype(int)
    kn = u[lo] + (t - lo) * (u[hi] - u[lo])
    kn[0], kn[-1] = u[0], u[-1]
    return kn


def basis(kn):
    """F (k x k: B^-1 D with a zero first and last row) and the penalty S = D^T B^-1 D of the knots (Wood, 4.1.2)."""
    kn = np.asarray(kn, dtype=np.float64)
    k = len(kn)
    h = np.diff(kn)
    D, B = np.zeros((k - 2, k)), np.zeros((k - 2, k - 2))
    for i in range(k - 2):
        D[i, i], D[i, i + 1], D[i, i + 2] = 1 / h[i], -1 / h[i] - 1 / h[i + 1], 1 / h[i + 1]
        B[i, i] = (h[i] + h[i + 1]) / 3
        if i + 1 < k - 2:
            B[i, i + 1] = B[i + 1, i] = h[i + 1] / 6
    BinvD = np.linalg.solve(B, D) if k > 2 else np.zeros((0, k))
    F = np.vstack([np.zeros((1, k)), BinvD, np.zeros((1, k))])
    return F, D.T @ BinvD


def design(kn, F, m):
    kn, m = np.asarray(kn, dtype=np.float64), np.asarray(m, dtype=np.float64)
    k = len(kn)
    j = np.clip(np.searchsorted(kn, m, side="right") - 1, 0, k - 2)
    h = kn[j + 1] - kn[j]
    xm, xp = kn[j + 1] - m, m - kn[j]
    X = ((xm ** 3 / h - h * xm) / 6)[:, None] * F[j] + ((xp ** 3 / h - h * xp) / 6)[:, None] * F[j + 1]
    X[np.arange(len(m)), j] += xm / h
    X[np.arange(len(m)), j + 1] += xp / h
    return X


def spectrum(X, S, v):
    """What GCV(lambda) is a function of: n, sum (v - vbar)^2, s (the two smallest exactly 0), z."""
    vc = v - v.mean()
    L = np.linalg.cholesky(X.T @ X)
    Li = np.linalg.inv(L)
    M = Li @ S @ Li.T
    s, U = np.linalg.eigh((M + M.T) / 2)
    s = np.maximum(s, 0.0)
    s[:min(2, len(s))] = 0.0
    return {"n": len(v), "syy": float(vc @ vc), "s": s, "z": U.T @ (Li @ (X.T @ vc))}


def gcv_spectral(sp, lam):
    g = np.where(sp["s"] == 0, 1.0, 1.0 / (1.0 + lam * sp["s"]))
    tr = float(g.sum())
    rss = sp["syy"] - float((sp["z"] ** 2 * (2 * g - g * g)).sum())
    den = sp["n"] - tr
    return (sp["n"] * rss / den ** 2 if den > 0 else np.inf), tr, rss


def search_lambda(sp):
    """The fixed search: the first smallest of the 97 grid points, 60 golden-section steps on its two neighbours."""
    f = lambda rho: gcv_spectral(sp, math.exp(rho))[0]
    vals = [f(r) for r in RHO_GRID]
    best = int(np.argmin(vals)) if np.isfinite(vals).any() else 0
    if best in (0, 96):
        return math.exp(RHO_GRID[best])
    phi = (math.sqrt(5.0) - 1.0) / 2.0
    lo, hi = RHO_GRID[best - 1], RHO_GRID[best + 1]
    c, d = hi - phi * (hi - lo), lo + phi * (hi - lo)
    fc, fd = f(c), f(d)
    for _ in range(60):
        if fc < fd:
            hi, d, fd = d, c, fc
            c = hi - phi * (hi - lo)
            fc = f(c)
        else:
            lo, c, fc = c, d, fd
            d = lo + phi * (hi - lo)
            fd = f(d)
    return math.exp(0.5 * (lo + hi))


def penalised_fit(X, S, v, lam):
    """argmin |v - X b|^2 + lam b^T S b by the augmented least-squares problem; the fitted values."""
    e, V = np.linalg.eigh((S + S.T) / 2)
    R = np.sqrt(np.maximum(e, 0.0))[:, None] * V.T
    Xa = np.vstack([X, math.sqrt(lam) * R])
    b = np.linalg.lstsq(Xa, np.concatenate([v, np.zeros(len(R))]), rcond=None)[0]
    return X @ b


def gcv_dense(X, S, v, lam):
    """GCV, tr A and RSS at lam from the influence matrix itself."""
    n = len(v)
    A = X @ np.linalg.solve(X.T @ X + lam * S, X.T)
    r = v - A @ v
    tr = float(np.trace(A))
    return n * float(r @ r) / (n - tr) ** 2, tr, float(r @ r)


def fit(m, var, nobs, gam_k=5, min_gene_cells=0, sp=None):
    """Step 1 and 2: v, valid, fit (NaN at an invalid gene), res (-Inf there) and what the fit used."""
    m, var, nobs = np.asarray(m, dtype=np.float64), np.asarray(var, dtype=np.float64), np.asarray(nobs)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.log(var)
    valid = np.isfinite(v) & np.isfinite(m) & (nobs >= min_gene_cells)
    n = int(valid.sum())
    out = {"v": v, "valid": valid, "n": n, "fit": np.full(len(m), np.nan), "res": np.full(len(m), -np.inf), "basis": 0, "lambda": np.nan,
           "knots": None, "X": None, "S": None}
    if n == 0:
        return out
    mv, vv = m[valid], v[valid]
    kn = place_knots(mv, gam_k) if (gam_k >= 2 and not n < 1.5 * gam_k) else None
    if kn is None:                                           # the straight line (the mean where m is constant)
        u = len(np.unique(mv))
        A = np.column_stack([np.ones(n), mv - mv.mean()]) if u >= 2 else np.ones((n, 1))
        f = A @ np.linalg.lstsq(A, vv, rcond=None)[0]
        out.update({"basis": min(u, 2), "u": u})
    else:
        F, S = basis(kn)
        X = design(kn, F, mv)
        lam = search_lambda(spectrum(X, S, vv)) if sp is None else float(sp)
        f = penalised_fit(X, S, vv, lam)
        out.update({"basis": gam_k, "lambda": lam, "knots": kn, "X": X, "S": S, "u": len(np.unique(mv))})
    out["fit"][valid] = f
    out["res"][valid] = vv - f
    return out


# ------------------------------------------------------------------ the special functions (mpmath)
def _log_ibeta_sym(a, z):
    """log I_z(a, a) for 0 < z <= 1/2: z^a (1 - z)^a / (a B(a, a)) * 2F1(2a, 1; a + 1; z), a series of positive terms."""
    term, total, n = mp.mpf(1), mp.mpf(1), 0
    while True:
        term = term * (2 * a + n) / (a + 1 + n) * z
        n += 1
        total += term
        if term < total * mp.mpf(10) ** -45:
            break
    return a * (mp.log(z) + mp.log1p(-z)) - mp.log(a) - (2 * mp.loggamma(a) - mp.loggamma(2 * a)) + mp.log(total)


def log_pf_one(res, a):
    res, a = float(res), float(a)
    if not a > 0 or math.isnan(res):
        return math.nan
    if res == -math.inf:
        return 0.0
    if res == math.inf:
        return -math.inf
    a, r = mp.mpf(a), mp.mpf(abs(res))
    lp = _log_ibeta_sym(a, 1 / (1 + mp.exp(r)))
    return float(lp if res >= 0 else mp.log1p(-mp.exp(lp)))


def log_pf(res, a):
    res, a = np.broadcast_arrays(np.asarray(res, dtype=np.float64), np.asarray(a, dtype=np.float64))
    return np.array([log_pf_one(r, q) for r, q in zip(res.ravel(), a.ravel())]).reshape(res.shape)


def _log_P_series(a, y):
    """log P(a, y) = log(y^a e^-y / Gamma(a + 1) * sum y^n / ((a + 1) .. (a + n))), a series of positive terms."""
    term, total, n = mp.mpf(1), mp.mpf(1), 0
    while True:
        n += 1
        term = term * y / (a + n)
        total += term
        if term < total * mp.mpf(10) ** -48:
            break
    return a * mp.log(y) - y - mp.loggamma(a + 1) + mp.log(total)


def log_Q(a, y):
    """log of the upper regularised incomplete gamma Q(a, y) (mpf): 1 - the series of P below a + 1, the Legendre continued
    fraction above, evaluated from its tail at a depth doubled until 45 digits agree."""
    a, y = mp.mpf(a), mp.mpf(y)
    if y <= 0:
        return mp.mpf(0)
    if y < a + 1:
        return mp.log1p(-mp.exp(_log_P_series(a, y)))

    def cf(depth):
        t = mp.mpf(0)
        for i in range(depth, 0, -1):
            t = (-i * (i - a)) / (y + 2 * i + 1 - a + t)
        return y + 1 - a + t
    depth, prev = 64, None
    while True:
        cur = cf(depth)
        if prev is not None and abs(cur - prev) <= abs(cur) * mp.mpf(10) ** -45:
            break
        prev, depth = cur, depth * 2
    return a * mp.log(y) - y - mp.loggamma(a) - mp.log(cur)


def log_qchisq_one(lp, df):
    lp, df = float(lp), float(df)
    if not df > 0 or math.isnan(lp) or lp > 0:
        return math.nan
    if lp == 0:
        return 0.0
    if lp == -math.inf:
        return math.inf
    a, target = mp.mpf(df) / 2, mp.mpf(lp)
    y = None
    if lp > -700:                                            # a start good to some 1e-13: Newton squares that at every step
        import scipy.stats

        y0 = float(scipy.stats.chi2.isf(math.exp(lp), df) if lp < -math.log(2.0) else scipy.stats.chi2.ppf(-math.expm1(lp), df)) / 2
        y = mp.mpf(y0) if math.isfinite(y0) and y0 > 0 else None
    if y is None:
        f = lambda ly: log_Q(a, mp.exp(ly)) - target        # decreasing in ly = log y
        lo = hi = mp.log(a)
        step = mp.mpf(1)
        while f(lo) < 0:
            lo -= step
            step *= 2
        step = mp.mpf(1)
        while f(hi) > 0:
            hi += step
            step *= 2
        y = mp.exp(mp.findroot(f, (lo, hi), solver="illinois", tol=mp.mpf(10) ** -12, maxsteps=400, verify=False))
    lga = mp.loggamma(a)
    lower = lp > -math.log(2.0)                              # the lower tail is the smaller one: Newton on log P in log y
    lq = mp.log(-mp.expm1(target))
    for _ in range(12):
        lQ = log_Q(a, y)
        if lower:
            lP = mp.log(-mp.expm1(lQ)) if lQ < -1 else _log_P_series(a, y)
            dt = (lP - lq) / mp.exp(a * mp.log(y) - y - lga - lP)
            y, dy = y * mp.exp(-dt), abs(dt) * y
        else:                                                # d log Q / dy = -y^(a-1) e^-y / (Gamma(a) Q)
            dy = (lQ - target) / mp.exp((a - 1) * mp.log(y) - y - lga - lQ)
            y += dy
        if abs(dy) <= y * mp.mpf(10) ** -40:
            break
    else:
        raise ArithmeticError(f"log_qchisq({lp}, {df}) did not converge")
    return float(2 * y)


def log_qchisq(lp, df):
    lp = np.asarray(lp, dtype=np.float64)
    return np.array([log_qchisq_one(v, df) for v in lp.ravel()]).reshape(lp.shape)


# ------------------------------------------------------------------ BH, scale factor, selection
def bh_adjust_log(lp):
    """bh.adjust(x, log = TRUE), literally (reference R/dimensinalityReduction.R:294-308); log(n / i) by the C library's log."""
    lp = np.asarray(lp, dtype=np.float64)
    out = lp.copy()
    nai = np.flatnonzero(~np.isnan(lp))
    x = lp[nai]
    n = len(x)
    idx = np.argsort(x, kind="stable")
    q = x[idx] + np.array([math.log(n / (i + 1)) for i in range(n)])
    a = np.minimum.accumulate(q[::-1])[::-1] if n else q
    out[nai[idx]] = a
    return out


def gsf(qv, v, min_av=1e-3, max_av=1e3):
    qv, v = np.asarray(qv, dtype=np.float64), np.asarray(v, dtype=np.float64)
    c = np.where(qv > max_av, max_av, qv)                    # pmin / pmax: a NaN stays
    c = np.where(c < min_av, min_av, c)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = np.sqrt(c / np.exp(v))
    s[~np.isfinite(s)] = 0.0
    return s


def over_dispersed(m, var, nobs, N, gam_k=5, min_gene_cells=0, min_av=1e-3, max_av=1e3, sp=None, genes=None):
    """The whole table.  ``genes``: the rows whose lp and qv are taken by mpmath (None: all); the others hold NaN there."""
    r = fit(m, var, nobs, gam_k, min_gene_cells, sp)
    G = len(r["v"])
    pick = np.arange(G) if genes is None else np.asarray(genes)
    lp, qv = np.full(G, np.nan), np.full(G, np.nan)
    for g in pick:
        lp[g] = log_pf_one(r["res"][g], nobs[g] / 2.0)
        qv[g] = log_qchisq_one(lp[g], N - 1) / N
    r.update({"lp": lp, "qv": qv, "picked": pick})
    if genes is None:
        r["lpa"] = bh_adjust_log(lp)
        r["gsf"] = gsf(qv, r["v"], min_av, max_av)
    return r


def odgenes_rows(lp, lpa, n_odgenes=None):
    """R/dimensinalityReduction.R:105-112, then ascending."""
    lp, lpa = np.asarray(lp), np.asarray(lpa)
    with np.errstate(invalid="ignore"):
        od = np.flatnonzero(lpa < math.log(0.1))
    if n_odgenes is not None:
        if n_odgenes > len(od):
            od = np.argsort(lp, kind="stable")[:min(len(lp), n_odgenes)]      # order(): NA last
        else:
            od = od[:n_odgenes]
    return np.sort(od)


def moments(X):
    """var (n - 1) and nobs per row of the dense matrix."""
    X = np.asarray(X, dtype=np.float64)
    return X.var(axis=1, ddof=1), (X != 0).sum(axis=1).astype(np.int32)


# ------------------------------------------------------------------ fixtures
def moments_case(G, seed=0, ties=None, N=200):
    """m, var, nobs of G made-up genes on a smooth trend: some var = 0, some nobs = 0, some nobs small.  ties: the number of
    distinct m."""
    rng = np.random.default_rng(seed + G)
    m = rng.uniform(0.2, 6.0, G)
    if ties is not None:
        m = rng.permutation(np.sort(rng.uniform(0.2, 6.0, ties))[np.arange(G) % ties])
    var = np.exp(1.5 - 0.9 * m + 0.08 * m * m + rng.normal(0, 0.5, G))
    nobs = rng.integers(3, N + 1, G).astype(np.int32)
    if G >= 6:
        var[G // 3] = 0.0
        nobs[G // 2] = 0
        nobs[G - 2] = 1
        m[1] = m[4]
        var[2] = var[5]
    return m, var, nobs, N


@functools.lru_cache(maxsize=None)
def planted(seed=7, G=300, N=200, n_planted=25):
    """300 genes x 200 cells of negative-binomial counts on a smooth variance-against-ICF trend, 25 genes with inflated
    variance (a burst in a tenth of the cells).  Returns the dense counts and the planted rows."""
    rng = np.random.default_rng(seed)
    frac = rng.uniform(0.15, 0.95, G)                         # the share of cells a gene is seen in sets its ICF weight
    mu = 0.5 + 6.0 * frac
    X = np.zeros((G, N))
    for g in range(G):
        lam = rng.gamma(8.0, mu[g] / 8.0, N)
        X[g] = rng.poisson(lam) * (rng.uniform(size=N) < frac[g])
    hot = np.sort(rng.choice(G, n_planted, replace=False))
    for g in hot:
        cells = rng.choice(N, N // 10, replace=False)
        X[g, cells] += rng.poisson(60.0 * mu[g], len(cells)) + 20
    X[:, 0] = np.maximum(X[:, 0], 1)                          # no empty gene: gficf keeps every row at cell_proportion_min = 0
    return X, hot
