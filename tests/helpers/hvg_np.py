"""NumPy f64 oracle of libgficf_hvg.so: every step of include/gficf_hvg.h stated plainly (the local fit is O(n^2): every
point's weights over all points, h by ``np.partition``).  The yardstick of tests/test_hvg_gpu.py; tests/test_hvg_cpu.py holds
it to answers derived by hand."""
from __future__ import annotations

import numpy as np
from scipy.special import erfc

CANNOT = "the variance-mean trend cannot be fitted"


# ------------------------------------------------------------------ step 1
def moments(X):
    """Per-row moments of the dense genes x cells matrix X, two passes over the non-zero entries as the kernel takes them."""
    X = np.asarray(X, dtype=np.float64)
    G, N = X.shape
    mean, ss, nobs = np.zeros(G), np.zeros(G), np.zeros(G, dtype=np.int32)
    for g in range(G):
        v = X[g][X[g] != 0]
        nobs[g] = len(v)
        mean[g] = v.sum() / N
        ss[g] = ((v - mean[g]) * (v - mean[g])).sum() + (N - len(v)) * (mean[g] * mean[g])
    var = ss / (N - 1)
    sd = np.sqrt(var)
    with np.errstate(divide="ignore", invalid="ignore"):
        cv = sd / mean
        lx, ly = np.log10(mean), np.log10(cv)
    return {"mean": mean, "sd": sd, "var": var, "nobs": nobs, "cv": cv, "lx": lx, "ly": ly, "valid": np.isfinite(lx) & np.isfinite(ly)}


# ------------------------------------------------------------------ step 2
def wave_sum(terms):
    """The "wave sum" of the header: lane l of 64 adds the terms l, l + 64, ... in turn, then the lanes are combined l with
    l ^ 32, ^ 16, ... ^ 1.  In that order a sum has the kernel's bits."""
    n = len(terms)
    rows = max(-(-n // 64), 1)
    pad = np.zeros(rows * 64)
    pad[:n] = terms
    lanes = np.zeros(64)
    for row in pad.reshape(rows, 64):
        lanes = lanes + row
    d = 32
    while d >= 1:
        lanes = lanes[:d] + lanes[d:2 * d]
        d //= 2
    return float(lanes[0])


def local_fit(xs, ys, at, k, w=None, ret_h=False):
    """The weighted local quadratic of the header at every point of ``at`` from the points (xs, ys), any order: O(n^2), every
    point's distance to every evaluation point.  The points are put in ascending order (stably) and the moments are wave
    sums over the window |xs - x| <= h, every product formed as the header writes it: the value has the kernel's bits."""
    xs, ys, at = (np.asarray(v, dtype=np.float64) for v in (xs, ys, at))
    w = np.ones(len(xs)) if w is None else np.asarray(w, dtype=np.float64)
    o = np.argsort(xs, kind="stable")
    xs, ys, w = xs[o], ys[o], w[o]
    fit, hs = np.full(len(at), np.nan), np.zeros(len(at))
    for e, x in enumerate(at):
        d = np.abs(xs - x)
        h = np.partition(d, k - 1)[k - 1]
        hs[e] = h
        win = d <= h
        xw, yw = xs[win], ys[win]
        if h > 0:
            u = (xw - x) / h
            au = np.abs(u)
            c = 1.0 - au * au * au
            W = np.where(au < 1, c * c * c, 0.0)
        else:
            u, W = np.zeros(len(xw)), np.ones(len(xw))
        ww = w[win] * W
        w1 = ww * u
        w2 = w1 * u
        w3 = w2 * u
        w4 = w3 * u
        S = [wave_sum(v) for v in (ww, w1, w2, w3, w4)]
        T = [wave_sum(v) for v in (ww * yw, w1 * yw, w2 * yw)]
        if not S[0] > 0:
            continue
        tol = 1e-10 * S[0]
        l1, l2 = S[1] / S[0], S[2] / S[0]
        p1, a12, a22, r1, r2 = S[2] - l1 * S[1], S[3] - l1 * S[2], S[4] - l2 * S[2], T[1] - l1 * T[0], T[2] - l2 * T[0]
        if not h > 0 or p1 < tol:
            fit[e] = T[0] / S[0]
            continue
        m = a12 / p1
        p2 = a22 - m * a12
        if p2 < tol:
            fit[e] = (T[0] - S[1] * (r1 / p1)) / S[0]
            continue
        b2 = (r2 - m * r1) / p2
        b1 = (r1 - a12 * b2) / p1
        fit[e] = (T[0] - S[1] * b1 - S[2] * b2) / S[0]
    return (fit, hs) if ret_h else fit


def r_median(v):
    v = np.sort(np.asarray(v, dtype=np.float64))
    n = len(v)
    return v[n // 2] if n % 2 else (v[n // 2 - 1] + v[n // 2]) / 2.0


def bisquare(res, s):
    r = res / (6.0 * s)
    return np.maximum(1.0 - r * r, 0.0) ** 2


def robust_fit(xs, ys, k, iters=3, w=None):
    """Cleveland's loop: iters + 1 fits at the data.  Returns (fit, weights, s): the last round's, and the iters medians."""
    xs, ys = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    w = np.ones(len(xs)) if w is None else np.asarray(w, dtype=np.float64).copy()
    s = np.zeros(iters)
    fit = local_fit(xs, ys, xs, k, w)
    for it in range(iters):
        res = ys - fit
        s[it] = r_median(np.abs(res))
        if not s[it] > 0:
            break                                                         # the weights stay, and so does the fit
        w = bisquare(res, s[it])
        fit = local_fit(xs, ys, xs, k, w)
    return fit, w, s


# ------------------------------------------------------------------ step 3
def seq_len(a, b, by):
    return int(np.floor((b - a) / by + 1e-10)) + 1


def seq(a, b, by):
    """R's seq(a, b, by)."""
    return a + np.arange(seq_len(a, b, by), dtype=np.float64) * by


def gap_counts(lx, grid, half=0.05):
    lx = np.asarray(lx, dtype=np.float64)
    return np.array([int(((lx >= g - half) & (lx < g + half)).sum()) for g in grid], dtype=np.int32)


def trusted_range(G, g5, gap, yseq):
    """(cdx0, j0): the curve is fitted through the 0-based grid indices cdx0 + 1 .. j0 + 1."""
    dense = np.flatnonzero(gap > 0.005 * G)
    rise = np.flatnonzero((np.diff(yseq) > 0) & (g5[1:] > 0))
    j0 = int(rise[0]) if len(rise) else len(yseq) - 2
    if len(dense) == 0 or dense[0] > j0 or j0 - int(dense[0]) + 1 < 3:
        raise ValueError(CANNOT)
    return int(dense[0]), j0


# ------------------------------------------------------------------ step 4
def curve(x, b, a):
    return 0.5 * np.log10(b / x + a)


def nls(x, y, b=1.0, a=0.0):
    """Gauss-Newton as R's nls() runs it on y ~ 0.5 * log10(b / x + a).  Returns (b, a, accepted steps)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n, c = len(x), 0.5 / np.log(10.0)

    def state(b, a):
        t = b / x + a
        if not ((t > 0) & np.isfinite(t)).all():
            return None
        r = y - 0.5 * np.log10(t)
        return t, r, float((r * r).sum())

    t, r, dev = state(b, a)
    fac, yy = 1.0, float((y * y).sum())
    for it in range(501):
        j1, j2 = c / (x * t), c / t
        n1 = np.sqrt((j1 * j1).sum())
        q1v = j1 / n1
        r12 = (q1v * j2).sum()
        v = j2 - r12 * q1v
        n2 = np.sqrt((v * v).sum())
        if not n1 > 0 or not n2 > 1e-10 * np.sqrt((j2 * j2).sum()):
            raise ValueError(CANNOT + ": singular gradient")
        q2v = v / n2
        q1, q2 = (q1v * r).sum(), (q2v * r).sum()
        qq = q1 * q1 + q2 * q2
        with np.errstate(invalid="ignore", divide="ignore"):
            if dev <= 1e-26 * (yy + n) or np.sqrt(qq / (dev - qq)) < 1e-5:
                return float(b), float(a), it
        if it == 500:
            break
        da = q2 / n2
        db = (q1 - r12 * da) / n1
        while True:
            if fac < 1.0 / 1024.0:
                raise ValueError(CANNOT + ": step factor below 1/1024")
            new = state(b + fac * db, a + fac * da)
            if new is not None and new[2] <= dev:
                b, a = b + fac * db, a + fac * da
                t, r, dev = new
                fac = min(2.0 * fac, 1.0)
                break
            fac /= 2.0
    raise ValueError(CANNOT + ": no convergence")


# ------------------------------------------------------------------ step 5
def curve_distance(lx, ly, b, a, ret_all=False):
    """cvDist of every (lx, ly) against the curve on seq(min lx, max lx, 0.001).  ``ret_all``: also the nearest grid index, the
    sign and the margin between the smallest and the second smallest distance of the window."""
    lx, ly = np.asarray(lx, dtype=np.float64), np.asarray(ly, dtype=np.float64)
    g1 = seq(lx.min(), lx.max(), 0.001)
    with np.errstate(invalid="ignore", divide="ignore"):
        yf = 0.5 * np.log10(b / 10.0 ** g1 + a)
    out, index, sign, margin = np.zeros(len(lx)), np.zeros(len(lx), dtype=np.int32), np.zeros(len(lx)), np.zeros(len(lx))
    for i in range(len(lx)):
        cx = np.flatnonzero((g1 >= lx[i] - 0.2) & (g1 < lx[i] + 0.2))
        d = np.sqrt((g1[cx] - lx[i]) ** 2 + (yf[cx] - ly[i]) ** 2)
        t = int(np.nanargmin(d))
        j = cx[t]
        if g1[j] > lx[i]:
            s = -1.0
        else:
            s = 1.0 if yf[j] < ly[i] else -1.0
        index[i], sign[i] = j, s
        out[i] = np.log2(10.0 ** (s * d[t]))
        rest = np.delete(d, t)
        margin[i] = np.nanmin(rest) - d[t] if len(rest) else np.inf
    return (out, index, sign, margin) if ret_all else out


# ------------------------------------------------------------------ step 6
def bw_nrd0(v):
    v = np.asarray(v, dtype=np.float64)
    hi = np.std(v, ddof=1)
    q1, q3 = np.quantile(v, [.25, .75])
    lo = min(hi, (q3 - q1) / 1.34)
    lo = lo or hi or abs(v[0]) or 1.0
    return 0.9 * lo * len(v) ** (-0.2)


def density(v):
    """(bw, grid, dens): the exact Gaussian sums on the 512-point grid."""
    v = np.asarray(v, dtype=np.float64)
    bw = bw_nrd0(v)
    grid = np.linspace(v.min() - 3 * bw, v.max() + 3 * bw, 512)
    z = (grid[:, None] - v[None, :]) / bw
    return bw, grid, np.exp(-0.5 * z * z).sum(axis=1)


# ------------------------------------------------------------------ step 7
def pvalues(cvdist, mid):
    d2 = cvdist - mid
    tmp = np.concatenate([d2[d2 <= 0], np.abs(d2[d2 < 0])]) + mid
    mu = tmp.mean()
    sigma = np.sqrt(((tmp - mu) ** 2).mean())
    return mu, sigma, 0.5 * erfc((cvdist - mu) / (sigma * np.sqrt(2.0)))


def p_adjust_fdr(p):
    p = np.asarray(p, dtype=np.float64)
    n = len(p)
    o = np.argsort(-p, kind="stable")
    q = np.minimum(1.0, np.minimum.accumulate(n / np.arange(n, 0, -1, dtype=np.float64) * p[o]))
    out = np.empty(n)
    out[o] = q
    return out


# ------------------------------------------------------------------ the whole procedure
def var_genes_from_moments(mean, cv):
    """Steps 2 - 7.  Per-gene outputs hold NaN at the invalid genes."""
    mean, cv = np.asarray(mean, dtype=np.float64), np.asarray(cv, dtype=np.float64)
    G = len(mean)
    with np.errstate(divide="ignore", invalid="ignore"):
        lx, ly = np.log10(mean), np.log10(cv)
    valid = np.isfinite(lx) & np.isfinite(ly)
    n = int(valid.sum())
    k = int(np.floor(0.2 * n))
    if k < 4:
        raise ValueError("the local regression needs at least 20 genes")
    order = np.flatnonzero(valid)[np.argsort(lx[valid], kind="stable")]
    xs, ys = lx[order], ly[order]
    fit, w, s = robust_fit(xs, ys, k)
    g5 = seq(xs[0], xs[-1], 0.005)
    gap = gap_counts(xs, g5)
    yseq = local_fit(xs, ys, g5, k, w)
    if not np.isfinite(fit).all() or not np.isfinite(yseq).all():
        raise ValueError("the local regression has no weight left at a point")
    r = {"lx": lx, "ly": ly, "valid": valid, "n": n, "k": k, "s": s, "g5": g5, "gap": gap, "ySeq": yseq}
    r["cdx0"], r["j0"] = trusted_range(G, g5, gap, yseq)
    pts = np.arange(r["cdx0"] + 1, r["j0"] + 2)
    r["b"], r["a"], r["nls_iter"] = nls(10.0 ** g5[pts], yseq[pts])
    cvd = curve_distance(xs, ys, r["b"], r["a"])
    r["bw"], grid, dens = density(cvd)
    r["dens"], r["distMid"] = dens, float(grid[int(np.argmax(dens))])
    r["mu"], r["sigma"], P = pvalues(cvd, r["distMid"])
    for name, v in (("fit", fit), ("weights", w), ("cvDist", cvd), ("P", P), ("FDR", p_adjust_fdr(P))):
        full = np.full(G, np.nan)
        full[order] = v
        r[name] = full
    return r


def find_var_genes(X):
    """The whole procedure from the dense genes x cells matrix."""
    m = moments(X)
    r = var_genes_from_moments(m["mean"], m["cv"])
    r.update({k: m[k] for k in ("mean", "cv", "sd", "var", "nobs")})
    return r


def select_rows(fdr):
    """The rows findClusterMarkers(hvg = TRUE) keeps, in its order (R/deGenes.R:31-35)."""
    fdr = np.asarray(fdr, dtype=np.float64)
    o = np.argsort(fdr, kind="stable")                                    # NaN last, as R's order()
    sig = int((fdr[o] < .1).sum())
    return o[:sig] if sig > 1000 else o[:min(1000, len(o))]


def planted(G, seed):
    """The planted trend of the tests: mean = 10^U(0, 4), cv = sqrt(50 / mean + 0.05) * 10^N(0, 0.04), a random twentieth of
    the genes raised by 10^U(0.2, 0.6).  Returns (mean, cv, the raised genes)."""
    rng = np.random.default_rng(seed)
    x = 10.0 ** rng.uniform(0, 4, G)
    cv = np.sqrt(50.0 / x + 0.05) * 10.0 ** rng.normal(0, 0.04, G)
    up = np.sort(rng.choice(G, G // 20, replace=False))
    cv[up] *= 10.0 ** rng.uniform(0.2, 0.6, len(up))
    return x, cv, up
