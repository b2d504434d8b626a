"""Inputs of tests/test_nmf_cpu.py and tests/test_nmf_gpu.py."""
import functools

import numpy as np
import scipy.sparse as sp

U = 2.0 ** -52

# (k, M) of the solve.  The kernel holds coordinates l and l + 64 in lane l (k = 63 / 64 / 65 and 127 / 128 sit on both sides of
# a lane and of the second register), and a workgroup walks 16 rows at a time for k > 64 (M = 15 / 16 / 17) and 4 for k <= 64
# (M = 3 / 4 / 5, added for it).  The grid stops at one wide workgroup per compute unit (256 x 16 rows) and eight narrow ones
# (2048 x 4 rows): M = 4100 and M = 8200, added for it, give some workgroups a second round of rows.
SOLVE_SHAPES = ([(k, M) for k in (1, 2, 63, 64, 65, 127, 128) for M in (1, 15, 16, 17, 1025)]
                + [(2, 3), (2, 5), (63, 3), (63, 4), (63, 5), (64, 4), (65, 4100), (2, 8200)])


def solve_case(k, M, seed=0, warm=False):
    """(S, B, H0): S = X'X of a standard normal X (3 k + 2 rows), B = H S + noise for a sparse non-negative H."""
    r = np.random.default_rng(1000 * k + M + seed)
    X = r.standard_normal((3 * k + 2, k))
    S = X.T @ X
    Ht = r.random((M, k)) * (r.random((M, k)) < 0.4)
    B = Ht @ S + 0.1 * r.standard_normal((M, k))
    H0 = r.random((M, k)) * (r.random((M, k)) < 0.5) if warm else None
    return S, B, H0


def sparse_uniform(G, N, density, seed):
    r = np.random.default_rng(seed)
    A = sp.random(G, N, density=density, format="csc", random_state=r, data_rvs=r.random)
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def sparse_300x200():
    """300 genes x 200 cells at density 0.1."""
    return sparse_uniform(300, 200, 0.1, 7)


@functools.lru_cache(maxsize=None)
def long_gene_40x1100():
    """40 genes x 1100 cells at density 0.1 with gene 3 stored in every cell: the transposed side crosses a 1024-entry segment."""
    r = np.random.default_rng(11)
    D = np.asarray(sparse_uniform(40, 1100, 0.1, 11).todense())
    D[3] = 0.1 + r.random(1100)
    A = sp.csc_matrix(D)
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def planted():
    """A = W0 H0, 300 x 200 of rank 4, the factors uniform with 30 % / 50 % of their entries kept; the start of
    default_rng(0): (A as CSC, start)."""
    r = np.random.default_rng(42)
    Wp = r.random((300, 4)) * (r.random((300, 4)) < 0.3)
    Hp = r.random((4, 200)) * (r.random((4, 200)) < 0.5)
    A = sp.csc_matrix(Wp @ Hp)
    A.sort_indices()
    return A, np.random.default_rng(0).random((300, 4))


def product_bound(absA, absX, n_terms):
    """The componentwise bound of a sum of n products formed in any order against the same sum in another: n 2^-52 sum |a||x|."""
    return n_terms * U * np.asarray(absA @ absX)
