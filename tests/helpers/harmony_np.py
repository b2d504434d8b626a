"""NumPy float64 restatement of include/gficf_harmony.h, stage by stage, written from the header (not from the kernels): the
yardstick of the Harmony tests.  Sums are numpy's own (another order than the device's): a comparison allows for that with
``sum_bound``.  Also the generator and the two figures of the quality condition."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -53


def phi(levels, B):
    """The B x N one-hot matrix of the V x N global level ids."""
    levels = np.asarray(levels)
    P = np.zeros((B, levels.shape[1]))
    for v in range(levels.shape[0]):
        P[levels[v], np.arange(levels.shape[1])] = 1.0
    return P


def normalise(Z):
    n = np.sqrt((Z * Z).sum(axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(n[:, None] > 0, Z / n[:, None], 0.0)
    return out, int((n == 0).sum())


def start(Zc, Y0, init_iter):
    Y, lab = np.array(Y0, dtype=np.float64), np.zeros(len(Zc), dtype=np.int32)
    for _ in range(init_iter):
        lab = np.argmax(Zc @ Y.T, axis=1).astype(np.int32)       # the first maximum: the lowest k wins a tie
        for k in range(len(Y)):
            s = Zc[lab == k].sum(axis=0)
            n = np.sqrt((s * s).sum())
            if n > 0:
                Y[k] = s / n
    return Y, lab


def start_margin(Zc, Y):
    """The gap between a cell's two largest dot products with the centroids Y (inf for K = 1)."""
    dots = np.sort(Zc @ Y.T, axis=1)
    return dots[:, -1] - dots[:, -2] if dots.shape[1] > 1 else np.full(len(Zc), np.inf)


def dist(Y, Zc):
    return 2.0 * (1.0 - Y @ Zc.T)


def soft(D, sigma, fac=None):
    e = np.exp(-(D - D.min(axis=0)) / sigma)
    if fac is not None:
        e = e * fac
    return e / e.sum(axis=0)


def assign(Zc, levels, B, Y, sigma):
    P = phi(levels, B)
    R = soft(dist(Y, Zc), sigma)
    return R, R @ P.T, np.outer(R.sum(axis=1), P.mean(axis=1))


def centroids(R, Zc, Y):
    s = R @ Zc
    n = np.sqrt((s * s).sum(axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n[:, None] > 0, s / n[:, None], Y)


def round_(Zc, levels, B, Y, R, O, E, theta, sigma, perm, n_blocks):
    """One clustering round; returns new (R, O, E, Y) and leaves its arguments alone."""
    P = phi(levels, B)
    pr = P.mean(axis=1)
    R, O, E = R.copy(), O.copy(), E.copy()
    Y = centroids(R, Zc, Y)
    D = dist(Y, Zc)
    for blk in np.array_split(np.asarray(perm), n_blocks):
        if len(blk) == 0:
            continue
        Pb = P[:, blk]
        O -= R[:, blk] @ Pb.T
        E -= np.outer(R[:, blk].sum(axis=1), pr)
        fac = np.ones((len(Y), len(blk)))
        for v in range(levels.shape[0]):
            b = levels[v, blk]
            fac = fac * ((E[:, b] + 1.0) / (O[:, b] + 1.0)) ** theta[b]
        R[:, blk] = soft(D[:, blk], sigma, fac)
        O += R[:, blk] @ Pb.T
        E += np.outer(R[:, blk].sum(axis=1), pr)
    return R, O, E, Y


def objective_terms(Zc, levels, B, Y, R, O, E, theta, sigma):
    """The K x N terms of the objective (their sum is the objective, the sum of their magnitudes bounds its rounding)."""
    D = dist(Y, Zc)
    with np.errstate(invalid="ignore", divide="ignore"):
        ent = np.where(R > 0, R * np.log(R), 0.0)
    L = theta * np.log((O + 1.0) / (E + 1.0))                    # K x B
    pen = np.zeros_like(R)
    for v in range(levels.shape[0]):
        pen += L[:, levels[v]]
    return R * D, sigma * ent, sigma * R * pen


def objective(Zc, levels, B, Y, R, O, E, theta, sigma):
    return float(sum(t.sum() for t in objective_terms(Zc, levels, B, Y, R, O, E, theta, sigma)))


def correct(Z, levels, B, R, lamb):
    """(Zcorr, W (K, B + 1, d), clusters left out, the largest condition number of an A_k)."""
    Ps = np.vstack([np.ones((1, Z.shape[0])), phi(levels, B)])
    Zcorr, W, flat, cond = Z.copy(), np.zeros((len(R), B + 1, Z.shape[1])), 0, 1.0
    for k in range(len(R)):
        PR = Ps * R[k]
        A = PR @ Ps.T + np.diag(np.concatenate([[0.0], lamb]))
        try:
            if not np.isfinite(A).all():
                raise np.linalg.LinAlgError
            np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            flat += 1
            continue
        cond = max(cond, float(np.linalg.cond(A)))
        W[k] = np.linalg.solve(A, PR @ Z)
        W[k, 0] = 0.0
        Zcorr -= (Ps.T @ W[k]) * R[k][:, None]
    return Zcorr, W, flat, cond


def harmony(Z, levels, B, theta, lamb, sigma, Y0, perm, init_iter, max_iter_harmony, max_iter_kmeans, n_blocks, epsilon_cluster, epsilon_harmony):
    """The chain (stage 7).  The same keys as ``HipOps.harmony`` returns, with the arrays."""
    Zc, _ = normalise(Z)
    Y, _ = start(Zc, Y0, init_iter)
    R, O, E = assign(Zc, levels, B, Y, sigma)
    objs, used, iter_rounds, h, converged, Zcorr = [objective(Zc, levels, B, Y, R, O, E, theta, sigma)], 0, [], [], False, Z.copy()
    for it in range(1, max_iter_harmony + 1):
        t = 0
        while t < max_iter_kmeans:
            R, O, E, Y = round_(Zc, levels, B, Y, R, O, E, theta, sigma, perm[used], n_blocks)
            used, t = used + 1, t + 1
            objs.append(objective(Zc, levels, B, Y, R, O, E, theta, sigma))
            if t >= 3:
                old, new = sum(objs[-4:-1]), sum(objs[-3:])
                if (old - new) / abs(old) < epsilon_cluster:
                    break
        iter_rounds.append(t)
        Zcorr = correct(Z, levels, B, R, lamb)[0]
        Zc, _ = normalise(Zcorr)
        h.append(objs[-1])
        if it >= 2 and (h[-2] - h[-1]) / abs(h[-2]) < epsilon_harmony:
            converged = True
            break
    return {"Z": Zcorr, "Zc": Zc, "R": R, "Y": Y, "O": O, "E": E, "objective": np.array(objs), "iter_rounds": np.array(iter_rounds, dtype=np.int32),
            "iterations": len(iter_rounds), "rounds": used, "converged": converged, "h": np.array(h)}


def sum_bound(c, n, abs_terms):
    """What a sum of n terms may differ by between two orders of addition: c n 2^-53 sum |terms|."""
    return c * n * U * abs_terms


# ------------------------------------------------------------------ the quality condition
def quality_data(seed, N=600, d=10, C=4, B=3):
    r = np.random.default_rng(seed)
    cent = 3 * r.standard_normal((C, d))
    off = 1.5 * r.standard_normal((B, d))
    ct = r.integers(0, C, N)
    pb = r.dirichlet(2 * np.ones(B), size=C)
    b = np.array([r.choice(B, p=pb[c]) for c in ct])
    X = cent[ct] + off[b] + 0.7 * r.standard_normal((N, d))
    return X, ct, b


def quality(X, ct, b, k=15):
    """(share of the k exact euclidean neighbours of the cell's own type, share from another batch over its expectation under
    perfect mixing within the type)."""
    D = ((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(D, np.inf)
    nn = np.argsort(D, axis=1, kind="stable")[:, :k]
    same_type = (ct[nn] == ct[:, None]).mean()
    other = (b[nn] != b[:, None]).mean()
    expect = np.mean([((ct == ct[i]) & (b != b[i])).sum() / max((ct == ct[i]).sum() - 1, 1) for i in range(len(X))])
    return float(same_type), float(other / expect)
