"""numpy port of libgficf_transform.so, written from the formulas of include/gficf_transform.h (nothing of uwot's or umap-learn's
text is used): the same stages with the same seams.

    query_knn(X_train, Q, k)                              -> idx (1-based training ids), dist     (euclidean, brute force)
    memberships(dist, local_connectivity)                 -> sigma, rho, W        (f32, the device's order of operations)
    init_positions(idx, W, Y_train)                       -> Y0                   (f32, sums in column order)
    row_schedule(W)                                       -> the 32-bit schedule words, relative to each row's own maximum
    layout(idx, W, Y_train, Y0, n_epochs, ..., dtype)     -> Y after epochs [epoch_begin, epoch_end), in float32 or float64
    vote(idx, labels)                                     -> the majority label, ties to the class met first in the row
    transform(X_train, Y_train, Q, k, n_epochs, ...)      -> Y

The layout is vectorised over the new cells: step c of an epoch handles column c of every row in which it is due, which keeps
the order within a row (the only order there is: the cells are independent)."""
import numpy as np

from tests.helpers.umap_np import U64, _attract, _repulse, blobs, due, exact_knn, mix, schedule  # noqa: F401  (re-exported)


def query_knn(X_train, Q, k):
    """(idx 1-based M x k, dist M x k float32): euclidean, ties by the smaller index."""
    X, Qm = np.asarray(X_train, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    D = np.empty((len(Qm), len(X)), dtype=np.float32)
    for r in range(0, len(Qm), 256):
        D[r:r + 256] = np.sqrt(((Qm[r:r + 256, None, :] - X[None, :, :]) ** 2).sum(-1))
    order = np.argsort(D, axis=1, kind="stable")[:, :k]
    return (order + 1).astype(np.int32), np.take_along_axis(D, order, axis=1)


def memberships(dist, local_connectivity=1.0):
    """dist M x k.  All k columns count.  All arithmetic in float32, sums in column order."""
    f32 = np.float32
    d = np.maximum(np.asarray(dist, dtype=f32), f32(0))         # a distance rounded below 0 (cosine, correlation) counts as 0
    M, k = d.shape
    cp = max(0.0, float(local_connectivity) - 1.0)
    f = int(np.floor(cp))
    r = f32(cp - f)
    cnt = np.zeros(M, dtype=np.int64)
    nz_first, nz_lo, nz_hi, nz_max, rowsum = (np.zeros(M, dtype=f32) for _ in range(5))
    for c in range(k):
        rowsum = rowsum + d[:, c]
        pos = d[:, c] > 0
        cnt = cnt + pos
        nz_first = np.where(pos & (cnt == 1), d[:, c], nz_first)
        nz_lo = np.where(pos & (cnt == f), d[:, c], nz_lo)
        nz_hi = np.where(pos & (cnt == f + 1), d[:, c], nz_hi)
        nz_max = np.where(pos, np.maximum(nz_max, d[:, c]), nz_max)
    if f == 0:
        rho = np.where(cnt > 0, r * nz_first, f32(0))
    else:
        rho = np.where(cnt >= f, nz_lo, np.where(cnt > 0, nz_max, f32(0)))
        if r > 0:
            rho = np.where(cnt > f, nz_lo + r * (nz_hi - nz_lo), rho)
    rho = rho.astype(f32)
    target = np.log2(f32(k)).astype(f32)
    lo, hi, mid = np.zeros(M, dtype=f32), np.full(M, np.inf, dtype=f32), np.ones(M, dtype=f32)
    live = np.ones(M, dtype=bool)
    x = d - rho[:, None]
    for _ in range(64):
        psum = np.zeros(M, dtype=f32)
        with np.errstate(divide="ignore", invalid="ignore", under="ignore", over="ignore"):
            for c in range(k):
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
    sigma = np.maximum(mid, f32(1e-3) * (rowsum / f32(k))).astype(f32)       # the row's own mean, whatever rho is
    with np.errstate(divide="ignore", invalid="ignore", under="ignore", over="ignore"):
        W = np.where((x <= 0) | (sigma[:, None] == 0), f32(1), np.exp(-x / sigma[:, None])).astype(f32)
    return sigma, rho, W


def init_positions(idx, W, Y_train):
    f32 = np.float32
    idx, W, Yt = np.asarray(idx), np.asarray(W, dtype=f32), np.asarray(Y_train, dtype=f32)
    M, k = idx.shape
    sw, sx, sy, mx, my = (np.zeros(M, dtype=f32) for _ in range(5))
    for c in range(k):
        yj = Yt[idx[:, c] - 1]
        sw = sw + W[:, c]
        sx = sx + W[:, c] * yj[:, 0]
        sy = sy + W[:, c] * yj[:, 1]
        mx = mx + yj[:, 0]
        my = my + yj[:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        Y = np.where((sw > 0)[:, None], np.stack([sx / sw, sy / sw], 1), np.stack([mx / f32(k), my / f32(k)], 1))
    return Y.astype(f32)


def row_schedule(W):
    """q_ic = min(floor((double)w_ic / wmax_i * 2^32), 2^32 - 1), wmax_i the row's own maximum (a row of zeros never fires)."""
    w = np.asarray(W, dtype=np.float32).astype(np.float64)
    wmax = w.max(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(w > 0, np.floor(w / wmax * 4294967296.0), 0.0)
    return np.minimum(q, 4294967295.0).astype(U64)


def layout(idx, W, Y_train, Y0, n_epochs, a=1.0, b=1.0, gamma=1.0, learning_rate=1.0, negative_sample_rate=5, seed=0, query_offset=0,
           epoch_begin=0, epoch_end=None, dtype=np.float32):
    """Epochs [epoch_begin, epoch_end) of n_epochs.  a, b, gamma, learning_rate, Y_train and Y0 are rounded to float32 first (what
    the device is handed), then every operation runs in ``dtype``."""
    dt = np.dtype(dtype).type
    idx = np.asarray(idx, dtype=np.int64)
    M, k = idx.shape
    a, b, gamma, lr = (float(np.float32(v)) for v in (a, b, gamma, learning_rate))
    epoch_end = n_epochs if epoch_end is None else epoch_end
    Yt = np.asarray(Y_train, dtype=np.float32).astype(dt)
    N = len(Yt)
    q = row_schedule(W)
    Y = np.asarray(Y0, dtype=np.float32).astype(dt)
    cell = (np.arange(M, dtype=np.int64) + int(query_offset)).astype(U64)
    for n in range(epoch_begin, epoch_end):
        alpha = dt(np.float32(lr) * (np.float32(1) - np.float32(n) / np.float32(n_epochs)))
        kn = mix(U64((int(seed) + n) & 0xFFFFFFFFFFFFFFFF))
        for c in range(k):
            on = np.flatnonzero(due(q[:, c], n))
            if len(on) == 0:
                continue
            y = _attract(Y[on], Yt[idx[on, c] - 1], alpha, a, b, dt)            # one attraction: the trained cell does not move
            with np.errstate(over="ignore"):
                ke = mix(kn + cell[on] * U64(k) + U64(c))
            for s in range(int(negative_sample_rate)):
                with np.errstate(over="ignore"):
                    key = mix(ke + U64(s))
                jn = (((key >> U64(32)) * U64(N)) >> U64(32)).astype(np.int64)
                y = _repulse(y, Yt[jn], alpha, a, b, gamma, dt)                  # never skipped
            Y[on] = y
    return Y


def vote(idx, labels):
    """The class with the most votes among labels[idx - 1]; among classes that tie, the one whose first member comes first."""
    idx, labels = np.asarray(idx), np.asarray(labels)
    out = np.empty(len(idx), dtype=labels.dtype)
    for i, row in enumerate(labels[idx - 1]):
        best, best_n = row[0], 0
        for l in row:                                               # row order: a later class needs strictly more votes
            n = int((row == l).sum())
            if n > best_n:
                best, best_n = l, n
        out[i] = best
    return out


def transform(X_train, Y_train, Q, k, n_epochs, a=1.0, b=1.0, gamma=1.0, learning_rate=0.25, negative_sample_rate=5,
              local_connectivity=1.0, seed=0, dtype=np.float32):
    idx, dist = query_knn(X_train, Q, k)
    _, _, W = memberships(dist, local_connectivity)
    Y0 = init_positions(idx, W, Y_train)
    return layout(idx, W, Y_train, Y0, n_epochs, a, b, gamma, learning_rate, negative_sample_rate, seed, dtype=dtype)
