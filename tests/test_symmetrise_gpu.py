"""GPU: the symmetrisation that libgficf_umap.so and libgficf_tsne.so share (csrc/knn_symmetrise.h), where sharing it can go
wrong: the table column that belongs to a column of the weights, the combiner handed in, the scratch carved behind W.

Host recomputation.  P is recomputed on the host from the device's own W (UMAP's memberships) or Pc (t-SNE's conditionals) and
the table: for UMAP in numpy f32 with one rounding per operation, in the operand order of include/gficf_umap.h,
``mix * ((lo + hi) - lo * hi) + (1 - mix) * (lo * hi)`` with lo <= hi; for t-SNE in f64, ``(lo + hi) / (2 N)``, then cast.  Both
are exact by construction, so row pointers, columns and value bits must be equal: there is no tolerance.  The tables name no
point twice in a row, so a pair has at most one weight per direction and the recomputation needs no order of its own.

Tables (N, k): (2, 2), 4 items; (64, 2), 256 items, so that the item behind the last crosses into a second workgroup of the heads
and emit kernels; (65, 3); the 2 001-point hub table of tests/test_umap_gpu.py, one row of 2 000 entries.  The small ones are
chains (row i names i + 1, i + 2, ..: one direction only) with a few mutual pairs in the middle, so that at mix = 0 every head of
a one-directional pair is dropped and the rows before and behind the mutual pairs are empty.  For t-SNE the same tables, the
perplexity chosen so that floor(3 perplexity) + 1 = k."""
import numpy as np
import pytest
import scipy.sparse as sp

import gficf_amd
from tests.helpers import umap_cases as uc
from tests.helpers import umap_np as un

pytestmark = pytest.mark.gpu

PERPLEXITY = {2: 1.0 / 3.0, 3: 0.7, 15: 4.7}                        # floor(3 perplexity) + 1 = k


def chain_table(N, k, mutual=()):
    """Row i names i + 1 .. i + k - 1 (mod N) behind itself, at growing distances; for (a, b) in ``mutual`` row b's first
    neighbour is a instead (row a names b already when b = a + 1).  1-based ids, no id twice in a row.  A perplexity below 1
    (k = 2, 3) cannot be met, beta grows until only the nearest neighbour and its ties keep a conditional: every third row
    has all its neighbours at one distance, so that t-SNE's later columns carry entries too."""
    idx = (np.arange(N)[:, None] + np.arange(k)[None, :]) % N + 1
    for a, b in mutual:
        assert idx[a, 1] == b + 1 and a + 1 not in idx[b]
        idx[b, 1] = a + 1
    dist = (np.arange(k, dtype=np.float32)[None, :] * (1.0 + (np.arange(N) % 7)[:, None] / 8.0)).astype(np.float32)
    dist[::3, 1:] = dist[::3, 1:2]                                  # every third row: its neighbours at one distance
    return idx.astype(np.int32), dist


@pytest.fixture(scope="module")
def tables():
    return {
        "two": chain_table(2, 2),                                   # 0 <-> 1: the chain of two is mutual by itself
        "n64": chain_table(64, 2, [(10, 11), (40, 41)]),
        "n65": chain_table(65, 3, [(20, 21), (30, 31)]),
        "hub": uc.hub_table(*un.exact_knn(uc.hub_points(), 15)),
    }


def directed(idx_cols, W):
    """The dense N x N matrix of the directed weights: column c of W belongs to column c of idx_cols."""
    N = W.shape[0]
    A = np.zeros((N, N), dtype=np.float32)
    rows = np.repeat(np.arange(N), W.shape[1])
    keep = W.ravel() > 0
    A[rows[keep], idx_cols.ravel()[keep] - 1] = W.ravel()[keep]
    return A


def csr_of(V):
    P = sp.csr_matrix(V)                                            # row by row, columns ascending
    P.eliminate_zeros()
    return P


def same_bits(P, E):
    assert P.dtype == np.float32 and E.dtype == np.float32
    assert np.array_equal(P.indptr, E.indptr) and np.array_equal(P.indices, E.indices)
    assert np.array_equal(P.data.view(np.uint32), E.data.view(np.uint32))


def umap_by_hand(A, mix):
    mix = np.float32(mix)
    lo, hi = np.minimum(A, A.T), np.maximum(A, A.T)
    prod = lo * hi
    return mix * ((lo + hi) - prod) + (np.float32(1) - mix) * prod  # f32 throughout, one rounding per operation


def tsne_by_hand(A):
    lo, hi = np.minimum(A, A.T).astype(np.float64), np.maximum(A, A.T).astype(np.float64)
    return ((lo + hi) / (2.0 * A.shape[0])).astype(np.float32)


@pytest.mark.parametrize("mix", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("name", ["two", "n64", "n65", "hub"])
def test_umap_graph_is_the_host_recomputation(tables, name, mix):
    idx, dist = tables[name]
    P, _, _, W = gficf_amd.fuzzy_simplicial_set(idx, dist, mix, ret_memberships=True)
    assert W.shape == idx.shape and (W[:, 0] == 0).all()            # the self column stays in W
    E = csr_of(umap_by_hand(directed(idx, W), mix))
    same_bits(P, E)
    deg = np.diff(P.indptr)
    if name == "hub":
        assert deg.max() == (2000 if mix > 0 else 14)               # the origin names 14 points back
    elif name != "two" and mix == 0:                                # the mutual pairs alone: empty rows before, between and behind
        assert P.nnz == 4 and deg[0] == 0 and deg[-1] == 0
    else:
        assert P.nnz > 0


@pytest.mark.parametrize("name", ["two", "n64", "n65", "hub"])
def test_tsne_affinities_are_the_host_recomputation(tables, name):
    idx, dist = tables[name]
    k = idx.shape[1]
    P, _, Pc = gficf_amd.tsne_affinities(idx, dist, PERPLEXITY[k], ret_cond=True)
    assert Pc.shape == (idx.shape[0], k - 1) and (Pc > 0).any(axis=0).all()     # no self column in Pc; every column is in use
    E = csr_of(tsne_by_hand(directed(idx[:, 1:], Pc)))
    same_bits(P, E)
    assert P.nnz > 0


def test_column_offset():
    """Column c of a row names i + 11 c (mod 67): an id read from a neighbouring column of the table is in nobody's row."""
    N, k = 67, 3
    idx = ((np.arange(N)[:, None] + 11 * np.arange(k)[None, :]) % N + 1).astype(np.int32)
    dist = np.tile(np.array([0, 1, 1], dtype=np.float32), (N, 1))   # a tie: both neighbours keep a conditional at perplexity < 1
    named = [set(idx[i, 1:] - 1) for i in range(N)]
    for P in (gficf_amd.fuzzy_simplicial_set(idx, dist)[0], gficf_amd.tsne_affinities(idx, dist, PERPLEXITY[k])[0]):
        assert P.nnz == 2 * N * (k - 1)                             # no pair is mutual here
        for i in range(N):
            for j in P.indices[P.indptr[i]:P.indptr[i + 1]]:
                assert j in named[i] or i in named[j], (i, j)
        T = P.T.tocsr()
        T.sort_indices()
        same_bits(P, T)


def test_degenerate_table():
    """Every column of every row names the row itself: no membership, no conditional, hence an empty matrix and no error (what
    the libraries returned before the symmetrisation was shared, too)."""
    N, k = 65, 3
    idx = np.tile(np.arange(1, N + 1, dtype=np.int32)[:, None], (1, k))
    dist = np.zeros((N, k), dtype=np.float32)
    P, _, _, W = gficf_amd.fuzzy_simplicial_set(idx, dist, ret_memberships=True)
    assert (W == 0).all() and P.nnz == 0 and (P.indptr == 0).all() and P.shape == (N, N)
    P, _, Pc = gficf_amd.tsne_affinities(idx, dist, PERPLEXITY[k], ret_cond=True)
    assert (Pc == 0).all() and P.nnz == 0 and (P.indptr == 0).all() and P.shape == (N, N)
