"""A numpy port of libgficf_tsne.so as include/gficf_tsne.h states it: the perplexity bisection and the symmetrisation, the
gradient in Rtsne's form (no factor 4) with the EXACT repulsion, dense O(N^2), and the stateless iteration rule.  ``dtype``
switches the arithmetic of the gradient and of the update between float32 and float64; the f64 run is the yardstick of
tests/test_tsne_gpu.py, the f32 run measures what a legitimate difference in precision amounts to (tests/helpers/tsne_cases.py).

No GPU, no library: numpy and scipy only."""
import numpy as np
import scipy.sparse as sp

MAX_STEPS = 200
TOL = 1e-5


# ------------------------------------------------------------------------------------------------ affinities
def row_entropy(x, beta):
    """(H, p / sum p) of one row: x the shifted squared distances of the entries that count."""
    p = np.exp(-beta * x)
    s = p.sum()
    return beta * (x * p).sum() / s + np.log(s), p / s


def conditionals(idx, dist, perplexity):
    """(beta N f64, Pc N x K f32) from the N x (K + 1) table: bhtsne's loop on the distances shifted by the row's smallest."""
    idx = np.asarray(idx)
    N, k = idx.shape
    K = k - 1
    d2 = np.asarray(dist, dtype=np.float32).astype(np.float64)[:, 1:] ** 2
    keep = idx[:, 1:] != np.arange(1, N + 1)[:, None]
    beta_out = np.ones(N)
    Pc = np.zeros((N, K), dtype=np.float32)
    target = np.log(perplexity)
    for i in range(N):
        x = d2[i, keep[i]]
        if len(x) == 0:
            continue
        x = x - x.min()
        beta, lo, hi = 1.0, -np.inf, np.inf
        for it in range(MAX_STEPS):
            H, p = row_entropy(x, beta)
            diff = H - target
            if abs(diff) < TOL or it == MAX_STEPS - 1:
                break
            if diff > 0:
                lo = beta
                beta = beta * 2.0 if np.isinf(hi) else (beta + hi) * 0.5
            else:
                hi = beta
                beta = beta * 0.5 if np.isinf(lo) else (beta + lo) * 0.5
        beta_out[i] = beta
        Pc[i, keep[i]] = p.astype(np.float32)
    return beta_out, Pc


def symmetrise(idx, Pc):
    """P = (Pc + Pc') / (2 N) as CSR float32, columns ascending, zeros dropped: one rounding of the f64 value."""
    idx = np.asarray(idx)
    N, k = idx.shape
    rows = np.repeat(np.arange(N), k - 1)
    cols = idx[:, 1:].ravel().astype(np.int64) - 1
    v = np.asarray(Pc, dtype=np.float32).ravel().astype(np.float64)
    A = sp.csr_matrix((v[v > 0], (rows[v > 0], cols[v > 0])), shape=(N, N))
    S = ((A + A.T) / (2.0 * N)).tocsr()
    S.sort_indices()
    P = sp.csr_matrix((S.data.astype(np.float32), S.indices.astype(np.int32), S.indptr.astype(np.int64)), shape=(N, N))
    P.eliminate_zeros()
    return P


def affinities(idx, dist, perplexity):
    beta, Pc = conditionals(idx, dist, perplexity)
    return symmetrise(idx, Pc), beta, Pc


# ------------------------------------------------------------------------------------------------ gradient
def _pairs(Y, dt):
    Y = np.asarray(Y).astype(dt)
    dx = Y[:, None, 0] - Y[None, :, 0]
    dy = Y[:, None, 1] - Y[None, :, 1]
    q = dt(1) / (dt(1) + (dx * dx + dy * dy))
    np.fill_diagonal(q, 0)
    return dx, dy, q


def _entries(P, Y, dt):
    P = sp.csr_matrix(P)
    Y = np.asarray(Y).astype(dt)
    d = Y[np.repeat(np.arange(P.shape[0]), np.diff(P.indptr))] - Y[P.indices]
    s = dt(1) + (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    return P.indptr, d, s, P.data.astype(dt)


def _row_sums(indptr, v, dt):
    """sum of v per row of the CSR layout, added in dt."""
    out = np.zeros(len(indptr) - 1, dtype=dt)
    ne = np.diff(indptr) > 0
    if ne.any():
        out[ne] = np.add.reduceat(v.astype(dt), indptr[:-1][ne])
    return out


def gradient(P, Y, exaggeration=1.0, dtype=np.float64, sums=False):
    """{"grad", "rep", "attr", "Z", "kl"} at Y; with ``sums`` also the sums of the absolute values of the terms of rep, attr
    (N x 2 each) and Z ("rep_abs", "attr_abs", "Z_abs" = Z): what an error bound per rounding multiplies."""
    dt = dtype
    dx, dy, q = _pairs(Y, dt)
    Z = q.sum(dtype=dt)
    q2 = q * q
    rep = np.stack([(q2 * dx).sum(axis=1, dtype=dt), (q2 * dy).sum(axis=1, dtype=dt)], axis=1)
    ptr, d, s, p = _entries(P, Y, dt)
    pq = p / s
    attr = np.stack([_row_sums(ptr, pq * d[:, 0], dt), _row_sums(ptr, pq * d[:, 1], dt)], axis=1)
    grad = (dt(exaggeration) * attr - rep / Z).astype(dt)
    p64, s64 = p.astype(np.float64), s.astype(np.float64)
    kl = float((p64 * np.log(p64 * float(Z) * s64)).sum())
    out = {"grad": grad, "rep": rep, "attr": attr, "Z": float(Z), "kl": kl}
    if sums:
        out["rep_abs"] = np.stack([(q2 * np.abs(dx)).sum(axis=1), (q2 * np.abs(dy)).sum(axis=1)], axis=1)
        out["attr_abs"] = np.stack([_row_sums(ptr, pq * np.abs(d[:, 0]), dt), _row_sums(ptr, pq * np.abs(d[:, 1]), dt)], axis=1)
        out["Z_abs"] = float(Z)
    return out


def kl_divergence(P, Y):
    """sum over the stored entries of P log(P / Q), Q = q / Z, in f64 (what the gradient is the gradient of, up to the factor 4)."""
    return gradient(P, Y)["kl"]


# ------------------------------------------------------------------------------------------------ layout
def schedule(n, stop_lying_iter, mom_switch_iter, momentum, final_momentum, exaggeration_factor):
    """(x, mu) in force in iteration n (0-based)."""
    return (exaggeration_factor if n < stop_lying_iter else 1.0), (momentum if n < mom_switch_iter else final_momentum)


def step(P, Y, uY, gains, x, mu, eta, dt):
    """One iteration on arrays of dtype dt; returns the new three."""
    dC = gradient(P, Y, x, dt)["grad"]
    gains = np.where(np.sign(dC) != np.sign(uY), gains + dt(0.2), gains * dt(0.8)).astype(dt)
    gains = np.maximum(gains, dt(0.01))
    uY = (dt(mu) * uY - (dt(eta) * gains) * dC).astype(dt)
    Y = (Y + uY).astype(dt)
    Y = (Y.astype(np.float64) - Y.astype(np.float64).mean(axis=0)).astype(dt)
    return Y, uY, gains


def layout(P, Y, max_iter=1000, iter_begin=0, iter_end=None, uY=None, gains=None, stop_lying_iter=250, mom_switch_iter=250, momentum=0.5,
           final_momentum=0.8, eta=200.0, exaggeration_factor=12.0, dtype=np.float32):
    """Iterations [iter_begin, iter_end) of max_iter; returns (Y, uY, gains) in dtype.  The state handed in is taken as float32
    values (what the library is handed), whatever the dtype of the arithmetic."""
    dt = dtype
    iter_end = max_iter if iter_end is None else iter_end
    assert 0 <= iter_begin <= iter_end <= max_iter
    N = len(Y)
    Y = np.asarray(Y, dtype=np.float32).astype(dt)
    uY = np.zeros((N, 2), dt) if uY is None else np.asarray(uY, dtype=np.float32).astype(dt)
    gains = np.ones((N, 2), dt) if gains is None else np.asarray(gains, dtype=np.float32).astype(dt)
    for n in range(iter_begin, iter_end):
        x, mu = schedule(n, stop_lying_iter, mom_switch_iter, momentum, final_momentum, exaggeration_factor)
        Y, uY, gains = step(P, Y, uY, gains, x, mu, eta, dt)
    return Y, uY, gains


def initial(N, seed):
    """The mirror's start: default_rng(seed).standard_normal((N, 2)) * 1e-4."""
    return np.random.default_rng(seed).standard_normal((N, 2)) * 1e-4


def normalize_input(X):
    """Rtsne's normalize_input: the columns centred, then everything divided by the largest magnitude."""
    X = np.array(X, dtype=np.float64, order="F")
    X -= X.mean(axis=0)
    top = np.abs(X).max()
    return X / top if top > 0 else X
