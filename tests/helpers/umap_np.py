"""numpy port of libgficf_umap.so, written from the formulas of include/gficf_umap.h (nothing of uwot's or umap-learn's text is
used): the same three stages with the same seams.

    smooth_knn(idx, dist, local_connectivity)            -> sigma, rho, W        (f32, the device's order of operations)
    symmetrise(idx, W, set_op_mix_ratio)                 -> P  (scipy CSR, f32, columns ascending, P == P.T bit for bit)
    fuzzy_graph(idx, dist, ...)                          -> P, sigma, rho
    schedule(val) / due(q, n)                            -> the 32-bit schedule words / which entries fire in epoch n
    layout(P, Y0, n_epochs, ..., dtype)                  -> Y after epochs [epoch_begin, epoch_end), in float32 or float64
    umap(X-free chain: idx, dist, Y0, ...)               -> Y

The layout sweep is vectorised over the vertices by row position: step p of an epoch handles the p-th entry of every row that
has one, which keeps the order within a row (the only order the owner-computes rule depends on).

quality(): trustworthiness and neighbour purity, the two figures the full-run tests compare."""
import numpy as np
import scipy.sparse as sp

U64 = np.uint64
_M1, _M2 = U64(0xBF58476D1CE4E5B9), U64(0x94D049BB133111EB)


def mix(z):
    """The splitmix64 finaliser on uint64 arrays (wrapping)."""
    z = np.asarray(z, dtype=U64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U64(30))) * _M1
        z = (z ^ (z >> U64(27))) * _M2
    return z ^ (z >> U64(31))


# ------------------------------------------------------------------------------------------------ graph
def smooth_knn(idx, dist, local_connectivity=1.0):
    """idx N x k (1-based), dist N x k.  All arithmetic in float32, sums in column order."""
    f32 = np.float32
    idx = np.asarray(idx)
    d = np.maximum(np.asarray(dist, dtype=f32), f32(0))         # a distance rounded below 0 (cosine, correlation) counts as 0
    N, k = d.shape
    f = int(np.floor(local_connectivity))
    r = f32(local_connectivity - f)
    cnt = np.zeros(N, dtype=np.int64)
    nz_lo, nz_hi, nz_max, rowsum = (np.zeros(N, dtype=f32) for _ in range(4))
    for c in range(k):
        rowsum = rowsum + d[:, c]
        if c >= 1:
            pos = d[:, c] > 0
            cnt = cnt + pos
            nz_lo = np.where(pos & (cnt == f), d[:, c], nz_lo)
            nz_hi = np.where(pos & (cnt == f + 1), d[:, c], nz_hi)
            nz_max = np.where(pos, np.maximum(nz_max, d[:, c]), nz_max)
    rho = np.where(cnt >= f, nz_lo, np.where(cnt > 0, nz_max, f32(0)))
    if r > 0:
        rho = np.where(cnt > f, nz_lo + r * (nz_hi - nz_lo), rho)
    rho = rho.astype(f32)
    target = np.log2(f32(k)).astype(f32)
    lo, hi, mid = np.zeros(N, dtype=f32), np.full(N, np.inf, dtype=f32), np.ones(N, dtype=f32)
    live = np.ones(N, dtype=bool)
    x = d - rho[:, None]
    for _ in range(64):
        psum = np.zeros(N, dtype=f32)
        with np.errstate(divide="ignore", invalid="ignore", under="ignore", over="ignore"):
            for c in range(1, k):
                psum = psum + np.where(x[:, c] > 0, np.exp(-x[:, c] / mid), f32(1)).astype(f32)
        live &= ~(np.abs(psum - target) < f32(1e-5))
        if not live.any():
            break
        up = live & (psum > target)
        dn = live & ~(psum > target)
        hi = np.where(up, mid, hi)
        lo = np.where(dn, mid, lo)
        with np.errstate(invalid="ignore", over="ignore"):
            half = ((lo + hi) * f32(0.5)).astype(f32)
        mid = np.where(up, half, np.where(dn, np.where(np.isinf(hi), mid * f32(2), half), mid)).astype(f32)
    gmean = f32(d.astype(np.float64).sum() / (N * k))
    floor_v = f32(1e-3) * np.where(rho > 0, rowsum / f32(k), gmean).astype(f32)
    sigma = np.maximum(mid, floor_v).astype(f32)
    own = np.arange(1, N + 1)[:, None]
    with np.errstate(divide="ignore", invalid="ignore", under="ignore", over="ignore"):
        W = np.where(idx == own, f32(0), np.where((x <= 0) | (sigma[:, None] == 0), f32(1), np.exp(-x / sigma[:, None]))).astype(f32)
    return sigma, rho, W


def combine(x, y, m):
    """P from the two memberships of a pair, smaller first, in float32."""
    f32 = np.float32
    lo, hi = np.minimum(x, y).astype(f32), np.maximum(x, y).astype(f32)
    prod = lo * hi
    return (f32(m) * ((lo + hi) - prod) + (f32(1) - f32(m)) * prod).astype(f32)


def symmetrise(idx, W, set_op_mix_ratio=1.0):
    idx = np.asarray(idx)
    N, k = idx.shape
    rows = np.repeat(np.arange(N), k)
    cols = idx.ravel().astype(np.int64) - 1
    w = np.asarray(W, dtype=np.float32).ravel()
    keep = w > 0
    A = sp.csr_matrix((w[keep], (rows[keep], cols[keep])), shape=(N, N))
    S = (A + A.T).tocoo()                                        # the pattern
    a = np.asarray(A[S.row, S.col]).ravel().astype(np.float32)
    b = np.asarray(A[S.col, S.row]).ravel().astype(np.float32)
    v = combine(a, b, set_op_mix_ratio)
    ok = v > 0
    P = sp.csr_matrix((v[ok], (S.row[ok], S.col[ok])), shape=(N, N))
    P.sort_indices()
    return P


def fuzzy_graph(idx, dist, set_op_mix_ratio=1.0, local_connectivity=1.0):
    sigma, rho, W = smooth_knn(idx, dist, local_connectivity)
    return symmetrise(idx, W, set_op_mix_ratio), sigma, rho


# ------------------------------------------------------------------------------------------------ schedule
def schedule(val):
    """q_e = min(floor((double)w_e / wmax * 2^32), 2^32 - 1)."""
    w = np.asarray(val, dtype=np.float32).astype(np.float64)
    if len(w) == 0:
        return np.zeros(0, dtype=U64)
    q = np.floor(w / w.max() * 4294967296.0)
    return np.minimum(q, 4294967295.0).astype(U64)


def due(q, n):
    """Which entries fire in epoch n (0-based)."""
    q = np.asarray(q, dtype=U64)
    return (((U64(n) + U64(1)) * q) >> U64(32)) > ((U64(n) * q) >> U64(32))


# ------------------------------------------------------------------------------------------------ layout
def _clip(x, dt):
    return np.minimum(np.maximum(x, dt(-4)), dt(4))


def _attract(y, yj, alpha, a, b, dt):
    diff = y - yj
    d2 = diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if a == 1 and b == 1:
            coef = dt(-2) / (d2 + dt(1))
        else:
            pd = np.power(d2, dt(b))
            coef = ((dt(-2) * dt(a) * dt(b)) * pd) / (d2 * (dt(a) * pd + dt(1)))
    coef = np.where(d2 > 0, coef, dt(0)).astype(dt)
    return (y + alpha * _clip(coef[:, None] * diff, dt)).astype(dt)


def _repulse(y, yj, alpha, a, b, gamma, dt):
    diff = y - yj
    d2 = diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]
    g2b = dt(2) * dt(gamma) * dt(b)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if a == 1 and b == 1:
            coef = g2b / ((dt(0.001) + d2) * (d2 + dt(1)))
        else:
            pd = np.power(d2, dt(b))
            coef = g2b / ((dt(0.001) + d2) * (dt(a) * pd + dt(1)))
        step = _clip(coef[:, None] * diff, dt)
    step = np.where((d2 > 0)[:, None], step, dt(4)).astype(dt)
    return (y + alpha * step).astype(dt)


def layout(P, Y0, n_epochs, a=1.0, b=1.0, gamma=1.0, learning_rate=1.0, negative_sample_rate=5, seed=0, epoch_begin=0, epoch_end=None,
           dtype=np.float32):
    """Epochs [epoch_begin, epoch_end) of n_epochs.  a, b, gamma, learning_rate are rounded to float32 first (what the device
    is handed), then every operation runs in ``dtype``."""
    dt = np.dtype(dtype).type
    P = sp.csr_matrix(P)
    if not P.has_sorted_indices:
        P = P.sorted_indices()
    N = P.shape[0]
    a, b, gamma, lr = (float(np.float32(v)) for v in (a, b, gamma, learning_rate))
    epoch_end = n_epochs if epoch_end is None else epoch_end
    rowptr, col = P.indptr.astype(np.int64), P.indices.astype(np.int64)
    q = schedule(P.data)
    length = np.diff(rowptr)
    order = np.argsort(-length, kind="stable")                  # vertices by decreasing row length: step p takes a prefix
    sorted_len = length[order]
    Y = np.array(Y0, dtype=dt)
    for n in range(epoch_begin, epoch_end):
        alpha = dt(np.float32(lr) * (np.float32(1) - np.float32(n) / np.float32(n_epochs)))
        kn = mix(U64((int(seed) + n) & 0xFFFFFFFFFFFFFFFF))
        fire = due(q, n)
        Ynew = Y.copy()
        for p in range(int(sorted_len[0]) if N else 0):
            vs = order[: int(np.searchsorted(-sorted_len, -p, side="left"))]       # rows longer than p
            e = rowptr[vs] + p
            on = fire[e]
            vs, e = vs[on], e[on]
            if len(vs) == 0:
                continue
            y = Ynew[vs]
            yj = Y[col[e]]
            y = _attract(y, yj, alpha, a, b, dt)
            y = _attract(y, yj, alpha, a, b, dt)
            with np.errstate(over="ignore"):
                ke = mix(kn + e.astype(U64))
            for s in range(int(negative_sample_rate)):
                with np.errstate(over="ignore"):
                    key = mix(ke + U64(s))
                jn = (((key >> U64(32)) * U64(N)) >> U64(32)).astype(np.int64)
                moved = _repulse(y, Y[jn], alpha, a, b, gamma, dt)
                y = np.where((jn != vs)[:, None], moved, y)
            Ynew[vs] = y
        Y = Ynew
    return Y


def umap(idx, dist, Y0, n_epochs, a=1.0, b=1.0, gamma=1.0, learning_rate=1.0, negative_sample_rate=5, set_op_mix_ratio=1.0,
         local_connectivity=1.0, seed=0, dtype=np.float32):
    P, _, _ = fuzzy_graph(idx, dist, set_op_mix_ratio, local_connectivity)
    return layout(P, Y0, n_epochs, a, b, gamma, learning_rate, negative_sample_rate, seed, dtype=dtype), P


# ------------------------------------------------------------------------------------------------ inputs and figures of merit
def exact_knn(X, k):
    """(idx 1-based N x k, dist N x k float32): euclidean, the point itself first, ties by the smaller index."""
    X = np.asarray(X, dtype=np.float64)
    D = np.empty((len(X), len(X)), dtype=np.float32)
    for r in range(0, len(X), 256):
        D[r:r + 256] = np.sqrt(((X[r:r + 256, None, :] - X[None, :, :]) ** 2).sum(-1))
    order = np.argsort(D, axis=1, kind="stable")[:, :k]
    return (order + 1).astype(np.int32), np.take_along_axis(D, order, axis=1)


def blobs(n=1200, n_blobs=12, dim=20, centre_sd=3.0, seed=0):
    """The quality input: n points in n_blobs Gaussian blobs (unit variance) of dim dimensions, centres N(0, centre_sd^2)."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, centre_sd, size=(n_blobs, dim))
    labels = np.arange(n) % n_blobs
    return centres[labels] + rng.standard_normal((n, dim)), labels


def pca_plane(X):
    Xc = X - X.mean(axis=0)
    _, _, vt = np.linalg.svd(Xc, full_matrices=False)
    return Xc @ vt[:2].T


def quality(X, Y, labels, k=15):
    """(trustworthiness with k neighbours, the share of each point's k nearest neighbours in the plane that carry its label)."""
    from sklearn.manifold import trustworthiness

    Y = np.asarray(Y, dtype=np.float64)
    t = float(trustworthiness(X, Y, n_neighbors=k))
    D = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(D, np.inf)
    nn = np.argsort(D, axis=1, kind="stable")[:, :k]
    return t, float((labels[nn] == labels[:, None]).mean())
