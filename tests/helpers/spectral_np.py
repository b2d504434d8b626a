"""The numpy side of tests/test_spectral_cpu.py and tests/test_spectral_gpu.py: the dense operator S = D^-1/2 P D^-1/2 and its
``eigh``, the canonical sign, the ring with its closed form, and the components through scipy relabelled to the smallest id.
The device's vectors and values are held to defining properties and to ``eigh``, never to a second solver.  The numpy statement
of the block method in tests/helpers/spectral_block_np.py has another role: it bounds CONVERGENCE (a case is solvable by the
method within max_restarts, and in how many restarts), and checks no vector.

``python -m tests.helpers.spectral_np`` recomputes, on the CPU and with the port of tests/helpers/umap_np.py alone, the quality
figures that tests/test_spectral_gpu.py carries (PORT_QUALITY)."""
import functools

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

from tests.helpers import umap_np as un

QUALITY_SEEDS = (1, 2, 3, 4, 5)
QUALITY_EPOCHS = 200


def dense_operator(P):
    """(S, q0): S = D^-1/2 P D^-1/2 dense f64, d the row sums, q0 = sqrt(d) / |sqrt(d)| its eigenvector at 1."""
    A = sp.csr_matrix(P).astype(np.float64).toarray()
    d = A.sum(axis=1)
    assert (d > 0).all()
    s = 1.0 / np.sqrt(d)
    q0 = np.sqrt(d)
    return s[:, None] * A * s[None, :], q0 / np.linalg.norm(q0)


def spectrum(P):
    """(values, vectors, q0) of S by ``eigh``, DESCENDING; for a connected graph values[0] = 1 belongs to +-q0."""
    S, q0 = dense_operator(P)
    w, U = np.linalg.eigh(S)
    return w[::-1].copy(), U[:, ::-1].copy(), q0


def canonical_sign(V):
    """Every column signed so that its largest-magnitude entry is positive, the lowest index on ties (the PCA rule)."""
    V = np.array(V, dtype=np.float64)
    for c in range(V.shape[1]):
        if V[int(np.argmax(np.abs(V[:, c]))), c] < 0:
            V[:, c] = -V[:, c]
    return V


def residuals(P, vectors, values):
    """|S x - theta x|_2 per column, in f64 on the host."""
    S, _ = dense_operator(P)
    return np.linalg.norm(S @ vectors - vectors * np.asarray(values)[None, :], axis=0)


def ring(N, s):
    """N vertices on a ring, each joined to its s neighbours on either side with weight 1 (float32 CSR, sorted columns)."""
    i = np.repeat(np.arange(N), 2 * s)
    off = np.tile(np.concatenate([np.arange(1, s + 1), -np.arange(1, s + 1)]), N)
    P = sp.csr_matrix((np.ones(len(i), np.float32), (i, (i + off) % N)), shape=(N, N))
    P.sum_duplicates()
    P.sort_indices()
    return P


def ring_value(N, s, mode=1):
    """The eigenvalue of S on ring(N, s) at angular mode ``mode``: (1 / s) sum_{t = 1..s} cos(2 pi t mode / N)."""
    return float(np.cos(2.0 * np.pi * np.arange(1, s + 1) * mode / N).sum() / s)


def complete(N):
    P = sp.csr_matrix(np.ones((N, N), np.float32) - np.eye(N, dtype=np.float32))
    P.sort_indices()
    return P


def components(P):
    """(labels int32, n): labels[i] the smallest vertex id of i's component; (i, j) joins whether or not (j, i) is stored."""
    n, lab = connected_components(sp.csr_matrix(P), directed=False)
    smallest = np.full(n, P.shape[0], dtype=np.int64)
    np.minimum.at(smallest, lab, np.arange(P.shape[0]))
    return smallest[lab].astype(np.int32), int(n)


def subspace_gap(A, B):
    """The sine of the largest principal angle between the column spaces of A and B (orthonormal columns, same width)."""
    s = np.linalg.svd(A.T @ B, compute_uv=False)
    return float(np.sqrt(max(0.0, 1.0 - min(s.min(), 1.0) ** 2)))


def sine(x, u):
    """The sine of the angle between the unit vectors x and u (computed from the remainder, not from 1 - cos^2)."""
    return float(np.linalg.norm(x - u * (u @ x)))


def davis_kahan(values, l, residual):
    """The bound residual / gap on the sine between a vector with that residual and eigenvector l of the (descending) spectrum."""
    others = np.delete(values, l)
    return float(residual / np.abs(others - values[l]).min())


def outside_cluster(x, theta, w, U, delta):
    """The norm of the part of x outside the span of the eigenvectors U[:, i] with |w_i - theta| < delta, from the remainder (as
    ``sine``).  At most residual / delta for ANY delta: with x = sum c_i u_i, |S x - theta x|^2 = sum (w_i - theta)^2 c_i^2
    >= delta^2 x (the sum of c_i^2 over the eigenvectors outside)."""
    Uc = U[:, np.abs(np.asarray(w) - theta) < delta]
    return float(np.linalg.norm(x - Uc @ (Uc.T @ x)))


def subspace_sine(X, Ub):
    """|X - Ub Ub' X|_2, the sine of the largest angle between span(X) and span(Ub) for orthonormal X (from the remainder: it does
    not bottom out at 1e-8 as ``subspace_gap`` does).  Davis-Kahan: at most ``subspace_bound``."""
    return float(np.linalg.norm(X - Ub @ (Ub.T @ X), 2))


def subspace_bound(w, values, residuals):
    """|residuals|_2 / sep on ``subspace_sine(X, U[:, 1:b + 1])``, sep = min |theta_l - w_i| over the eigenvalues i that are not
    among the b leading non-trivial ones (the trivial one included).  With R = S X - X diag(theta) and U2 those eigenvectors,
    (U2' X)_il = (U2' R)_il / (w_i - theta_l), so |U2' X|_2 <= |U2' X|_F <= |R|_F / sep."""
    b = len(values)
    others = np.concatenate([w[:1], w[b + 1:]])
    sep = np.abs(others[:, None] - np.asarray(values)[None, :]).min()
    return float(np.linalg.norm(residuals) / sep)


# ------------------------------------------------------------------------------------------------ graphs of hubs and of threshold rows
HUB_LEN = 256                         # SP_HUB_LEN of spectral.hip: a longer row is multiplied by a whole wave from the hub list
HUB_WAVES = 1024                      # SP_HUB_WAVES: the waves that share the hub list, at most


def planted(N=1100, groups=9, seed=4):
    """The complete graph on N vertices without its diagonal, label = i % groups: weights uniform(0.5, 1) within a group and
    uniform(0.01, 0.1) across, symmetrised from the upper triangle.  Every row has N - 1 entries: N hub rows, more than the
    hub waves, and no row for the 8-lane path.  groups - 1 eigenvalues near 0.58, then a gap down to 0.02."""
    rng = np.random.default_rng(seed)
    label = np.arange(N) % groups
    inside, across = rng.uniform(0.5, 1.0, (N, N)), rng.uniform(0.01, 0.1, (N, N))
    W = np.triu(np.where(label[:, None] == label[None, :], inside, across), 1).astype(np.float32)
    P = sp.csr_matrix(W + W.T)
    P.sort_indices()
    return P


def threshold():
    """ring(600, 128) plus the edge (0, 300) both ways: 598 rows of exactly HUB_LEN entries (the longest the 8-lane path takes) and
    two of HUB_LEN + 1 (the shortest hubs).  Its spectrum comes in near-degenerate pairs."""
    P = ring(600, 128).tolil()
    P[0, 300] = P[300, 0] = 1.0
    P = P.tocsr().astype(np.float32)
    P.sort_indices()
    return P


# ------------------------------------------------------------------------------------------------ the connected blobs (case 2)
@functools.lru_cache(maxsize=None)
def connected_blobs():
    """(X, labels, idx, dist): un.blobs(1200, 12, 20, 1.0, 0) and its exact 15-neighbour table."""
    X, labels = un.blobs(1200, 12, 20, 1.0, 0)
    idx, dist = un.exact_knn(X, 15)
    return X, labels, idx, dist


def eigh_start(P, seed, jitter=True):
    """spectral_init's array from ``eigh`` instead of the library: the two vectors below the trivial one with the sign rule, scaled to
    10 plus the noise of the generator's second draw (the first is the start block, which ``eigh`` has no use for)."""
    _, U, _ = spectrum(P)
    rng = np.random.default_rng(seed)
    rng.standard_normal((P.shape[0], 2))
    Y = canonical_sign(U[:, 1:3])
    if jitter:
        Y = Y * (10.0 / np.abs(Y).max()) + rng.normal(0.0, 1e-4, size=Y.shape)
    return Y


def _main():
    X, labels, idx, dist = connected_blobs()
    P, _, _ = un.fuzzy_graph(idx, dist)
    print("components:", components(P)[1], "top of the spectrum:", spectrum(P)[0][:4])
    out = []
    for s in QUALITY_SEEDS:
        Y = un.layout(P, eigh_start(P, s), QUALITY_EPOCHS, seed=s)
        out.append(tuple(round(v, 5) for v in un.quality(X, Y, labels)))
    print(f"PORT_QUALITY = {out!r}")


if __name__ == "__main__":
    _main()
