"""Inputs, property checks and layout cases shared by tests/test_tsne_cpu.py (the numpy port) and tests/test_tsne_gpu.py (the
library), so that both are held to the same statements.

``python -m tests.helpers.tsne_cases`` recomputes, on the CPU and with the port alone, the MEASURED tables that
tests/test_tsne_gpu.py carries (the f32 / f64 deviation of every layout case, the port's quality figures);
``python -m tests.helpers.tsne_cases --golden`` rewrites the states of the 1 500-point cases under tests/golden/ first (the
port's f64 state at the iterations 249 and 600: about a minute of dense iterations that no test should repeat)."""
import functools
import os
import sys

import numpy as np
import scipy.sparse as sp

from tests.helpers import tsne_np as tn
from tests.helpers import umap_cases as uc
from tests.helpers import umap_np as un

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
PERPLEXITIES = (2, 5, 30, 42)                 # K = 6, 15, 90, 126: k = 127 is the last the search provides


# ------------------------------------------------------------------------------------------------ affinities
def affinity_input(name):
    """"graph": umap_cases.graph_input() (a block of 20 identical points, a row of one distance); "rand": 257 random points."""
    return uc.graph_input() if name == "graph" else uc.random_input()


def check_affinities(idx, dist, perplexity, P, beta, Pc):
    """Everything in f64 from the given beta and Pc: no second implementation in the loop.  Returns the rows that can reach the
    target."""
    idx = np.asarray(idx)
    N, k = idx.shape
    K = k - 1
    assert K == int(np.floor(3 * perplexity))
    beta, Pc = np.asarray(beta), np.asarray(Pc)
    assert beta.dtype == np.float64 and beta.shape == (N,) and Pc.dtype == np.float32 and Pc.shape == (N, K)
    assert np.isfinite(beta).all() and (beta > 0).all() and np.isfinite(Pc).all() and (Pc >= 0).all()
    d32 = np.asarray(dist, dtype=np.float32)[:, 1:]
    d2 = d32.astype(np.float64) ** 2
    keep = idx[:, 1:] != np.arange(1, N + 1)[:, None]
    assert (Pc[~keep] == 0).all()                                 # an entry whose id is the row itself
    reach = np.zeros(N, dtype=bool)
    for i in range(N):
        x = d2[i, keep[i]]
        x = x - x.min()
        m, n_min = len(x), int((d32[i, keep[i]] == d32[i, keep[i]].min()).sum())
        H, p = tn.row_entropy(x, beta[i])
        got = Pc[i, keep[i]].astype(np.float64)
        # Pc is p / sum p at the beta returned, rounded to f32 (values below the smallest normal f32 lose more, or vanish)
        assert (np.abs(got - p) <= 2.0 ** -24 * p + 2.0 ** -126).all(), i
        assert abs(got.sum() - 1.0) <= m * 2.0 ** -24, i
        # H runs from log(m) at beta = 0 down to log(n_min): the target is reachable strictly between the two
        reach[i] = n_min < perplexity < m
        if reach[i]:
            # the entropy of the f32 conditionals themselves: H moves by at most sum |dp| (|log p| + 1 + beta x), |dp| <= 2^-24 p
            slack = 2.0 ** -24 * float((p * (np.abs(np.log(np.maximum(p, 1e-300))) + 1.0 + beta[i] * x)).sum())
            assert abs(H - np.log(perplexity)) < 1e-5 + slack, (i, H, np.log(perplexity))
        if n_min == m:                                            # one distance only: uniform, exactly
            v = Pc[i, keep[i]]
            assert (v.view(np.uint32) == v.view(np.uint32)[0]).all(), i
            assert abs(float(v[0]) - 1.0 / m) <= np.spacing(np.float32(1.0 / m)), i
    # P against the conditionals it was made of
    rows = np.repeat(np.arange(N), K)
    cols = idx[:, 1:].ravel().astype(np.int64) - 1
    v = Pc.ravel().astype(np.float64)
    A = sp.csr_matrix((v[v > 0], (rows[v > 0], cols[v > 0])), shape=(N, N))
    E = ((A + A.T) / (2.0 * N)).tocsr()
    E.sort_indices()
    P = sp.csr_matrix(P)
    assert P.dtype == np.float32 and P.shape == (N, N)
    assert P.indptr[0] == 0 and P.indptr[-1] == len(P.indices) == len(P.data) <= 2 * N * K
    for i in range(N):
        c = P.indices[P.indptr[i]:P.indptr[i + 1]]
        assert (np.diff(c) > 0).all(), i                          # ascending, no repeats
        assert not (c == i).any(), i                              # no diagonal
    assert (P.data > 0).all()                                     # zeros dropped
    Ed, Pd = E.toarray(), P.astype(np.float64).toarray()         # (N is a few hundred here)
    assert (np.abs(Pd - Ed) <= 2.0 ** -23 * Ed + 2.0 ** -149).all()
    assert ((Pd != 0) | (Ed < 2.0 ** -148)).all()                # every entry that f32 can hold is stored
    PT = P.T.tocsr()
    PT.sort_indices()
    assert np.array_equal(PT.indptr, P.indptr) and np.array_equal(PT.indices, P.indices)
    assert np.array_equal(PT.data.view(np.uint32), P.data.view(np.uint32))         # P[i,j] and P[j,i]: the same bits
    assert abs(float(P.data.astype(np.float64).sum()) - 1.0) <= P.nnz * 2.0 ** -24
    return reach


def same_bits(A, B):
    return (np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
            and np.array_equal(A.data.view(np.uint32), B.data.view(np.uint32)))


# ------------------------------------------------------------------------------------------------ repulsion by counting
def counting_sizes(shape):
    """The N of the closed-form cases from ``shape`` = tsne_shape: below a tile, a tile +- 1, a row block +- 1, and three row
    blocks whose last one and whose last slice are ragged."""
    tile, rpb = shape["tile"], shape["rows_per_block"]
    return sorted({tile // 2 + 3, tile - 1, tile + 1, rpb - 1, rpb + 1, 2 * rpb + tile + tile // 2 + 5})


def two_sites(N):
    """Points with i mod 3 = 0 at (1, 0), the rest at (0, 0).  Returns (Y, Z, rep): the cross-site q is 1 / 2, so
    Z = n1 (n1 - 1) + n2 (n2 - 1) + n1 n2 and rep_i = (+-n_other / 4, 0), all exactly representable."""
    at1 = np.arange(N) % 3 == 0
    n1 = int(at1.sum())
    n2 = N - n1
    Y = np.zeros((N, 2), dtype=np.float32)
    Y[at1, 0] = 1.0
    rep = np.zeros((N, 2))
    rep[at1, 0] = n2 / 4.0
    rep[~at1, 0] = -n1 / 4.0
    return Y, float(n1 * (n1 - 1) + n2 * (n2 - 1) + n1 * n2), rep


def ring_graph(N):
    """A P with one entry per row: i -> (i + 1) mod N, the value 1 / N (not symmetric: the gradient entry does not ask)."""
    return sp.csr_matrix((np.full(N, 1.0 / N, dtype=np.float32), (np.arange(N) + 1) % N, np.arange(N + 1)), shape=(N, N))


# ------------------------------------------------------------------------------------------------ layout cases
LAYOUT_ITER = 1000
LAYOUT_SEED = 42
WINDOWS = {"0-1": (0, 1), "0-3": (0, 3), "249-252": (249, 252), "600-603": (600, 603)}
SETS = {"big": (1500, 30), "small": (257, 5)}                    # points, perplexity
GRADIENT_N = 1500


@functools.lru_cache(maxsize=None)
def layout_points(name):
    n, _ = SETS[name]
    return np.random.default_rng(7 if name == "big" else 5).standard_normal((n, 10))


@functools.lru_cache(maxsize=None)
def layout_graph(name):
    """P of the layout cases, made by the port from the exact table of layout_points(name)."""
    n, perp = SETS[name]
    idx, dist = un.exact_knn(layout_points(name), int(np.floor(3 * perp)) + 1)
    return tn.affinities(idx, dist, perp)[0]


def _golden_path(name, it):
    return os.path.join(GOLDEN, f"tsne_state_{name}_{it}.npy")


@functools.lru_cache(maxsize=None)
def state(name, it):
    """(Y, uY, gains) float32 handed to every run of a window that begins at iteration ``it``: the start for 0, else the port's
    f64 state, rounded.  The 1 500-point states are read from tests/golden/ (3 x N x 2 float32), the small ones are made here."""
    n, _ = SETS[name]
    if it == 0:
        return tn.initial(n, LAYOUT_SEED).astype(np.float32), np.zeros((n, 2), np.float32), np.ones((n, 2), np.float32)
    if name == "big":
        S = np.load(_golden_path(name, it))
        assert S.shape == (3, n, 2) and S.dtype == np.float32
        return S[0], S[1], S[2]
    return tuple(a.astype(np.float32) for a in _port_state(name, it))


def _port_state(name, it):
    n, _ = SETS[name]
    return tn.layout(layout_graph(name), tn.initial(n, LAYOUT_SEED), LAYOUT_ITER, 0, it, dtype=np.float64)


def port_window(name, window, dtype):
    lo, hi = WINDOWS[window]
    Y, uY, gains = state(name, lo)
    return tn.layout(layout_graph(name), Y, LAYOUT_ITER, lo, hi, uY, gains, dtype=dtype)


def layout_cases():
    return [(s, w) for s in SETS for w in WINDOWS]


def tolerance(measured, top):
    """8 x the port's own f32 / f64 deviation, never below 64 f32 roundings at the largest coordinate of the case."""
    return max(8.0 * measured, 64 * 2.0 ** -24 * top)


# ------------------------------------------------------------------------------------------------ quality
QUALITY_SEEDS = (1, 2, 3, 4, 5)
QUALITY_ITER = 1000
QUALITY_PERPLEXITY = 30


def _write_golden():
    os.makedirs(GOLDEN, exist_ok=True)
    n, _ = SETS["big"]
    P = layout_graph("big")
    Y, uY, gains = tn.initial(n, LAYOUT_SEED), None, None
    at = 0
    for it in sorted({lo for lo, _ in WINDOWS.values() if lo > 0}):
        Y, uY, gains = tn.layout(P, Y, LAYOUT_ITER, at, it, uY, gains, dtype=np.float64)
        # (the state continues from its float32 rounding: tn.layout takes what it is handed as float32, as the library does)
        np.save(_golden_path("big", it), np.stack([Y, uY, gains]).astype(np.float32))
        at = it
        print("wrote", _golden_path("big", it))


def _main():
    if "--golden" in sys.argv:
        _write_golden()
        state.cache_clear()
    print("MEASURED = {")
    for case in layout_cases():
        a, b = port_window(*case, np.float32), port_window(*case, np.float64)
        dev = float(np.abs(a[0].astype(np.float64) - b[0]).max())
        print(f"    {case!r}: ({dev:.3e}, {float(np.abs(b[0]).max()):.3e}),")
    print("}")
    if "--no-quality" in sys.argv:
        return
    X, labels, cells = uc.quality_input()
    Xn = tn.normalize_input(cells)
    idx, dist = un.exact_knn(Xn, 3 * QUALITY_PERPLEXITY + 1)
    P = tn.affinities(idx, dist, QUALITY_PERPLEXITY)[0]
    print("MEASURED_QUALITY = [")
    for s in QUALITY_SEEDS:
        Y, _, _ = tn.layout(P, tn.initial(len(Xn), s), QUALITY_ITER, dtype=np.float64)
        t, pur = un.quality(X, Y, labels)
        print(f"    ({t:.5f}, {pur:.5f}, {tn.kl_divergence(P, Y):.5f}),")
    print("]")


if __name__ == "__main__":
    _main()
