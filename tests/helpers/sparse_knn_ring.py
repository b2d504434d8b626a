"""An answer that is DERIVED, not computed, for the sparse neighbour search (the companion of closed_form.py): a ring of cells.

Cell i of N = G stores the w genes i, i + 1, ..., i + w - 1 (mod G) with value 1.  The cells i and i +- t share w - t genes for
t < w and none beyond, so with na = w for every cell
    euclidean  d = sqrt(2 w - 2 (w - t)) = sqrt(2 t)        cosine  d = 1 - (w - t) / w = t / w,
every operation of which is exact up to the square root and the one rounding to f32.  For k - 1 = 2 h neighbours with h < w the
neighbours of cell i are i +- 1, ..., i +- h, ordered by ring distance and then by id."""
import numpy as np
import scipy.sparse as sp


def ring_matrix(N, w):
    c = np.repeat(np.arange(N, dtype=np.int64), w)
    r = (c + np.tile(np.arange(w, dtype=np.int64), N)) % N
    M = sp.csc_matrix((np.ones(N * w), (r, c)), shape=(N, N))
    M.sort_indices()
    return M


def ring_expected(N, w, h, metric):
    """(idx 1-based int32, dist f64 of the f32 value), N x (2 h + 1)."""
    i = np.arange(N, dtype=np.int64)[:, None]
    t = np.arange(1, h + 1, dtype=np.int64)[None, :]
    lo, hi = np.minimum((i - t) % N, (i + t) % N), np.maximum((i - t) % N, (i + t) % N)
    idx = np.concatenate([i, np.stack([lo, hi], axis=2).reshape(N, 2 * h)], axis=1) + 1
    d = np.sqrt(2.0 * t) if metric == "euclidean" else t / float(w)
    dist = np.concatenate([[0.0], np.repeat(d.ravel(), 2)]).astype(np.float32).astype(np.float64)
    return idx.astype(np.int32), np.tile(dist, (N, 1))
