"""libgficf_sparse_knn.so on the device: find_nn_sparse against the NumPy oracle under the comparison rule of
tests/helpers/sparse_knn_oracle.py (all metrics and list lengths, the seams of the tile width that find_nn_sparse_shape reports,
the column lengths around the lane group's stride, ties and duplicates, candidate slices and query ranges), against a closed
form that needs no oracle (tests/helpers/sparse_knn_ring.py), and against the dense search find_nn on the same cells."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import gficf_amd
from gficf_amd import GficfError, _sparse_knn_lib
from tests.helpers import sparse_knn_oracle as so
from tests.helpers import sparse_knn_ring as ring

pytestmark = pytest.mark.gpu

KS = (1, 16, 64, 65, 128)


@functools.lru_cache(maxsize=None)
def _case(G, N, density, seed):
    return so.case(G, N, density, seed)


@functools.lru_cache(maxsize=None)
def _q(G, N, density, seed, metric):
    return so.q_and_scale(_case(G, N, density, seed), metric)


def _want(q, scale, metric, k):
    idx, dist = so.table(q, metric, k)
    return {"idx": idx, "dist": dist, "q": q, "scale": scale}


def _check(M, metric, k, **kw):
    got = gficf_amd.find_nn_sparse(M, k, metric=metric)
    q, scale = so.q_and_scale(M, metric)
    return got, so.compare(got, _want(q, scale, metric, k), metric, **kw)


# ------------------------------------------------------------------------------------------------ all metrics
@pytest.mark.parametrize("seed", (1, 2, 3))
@pytest.mark.parametrize("metric", so.METRICS)
def test_all_metrics_and_list_lengths(metric, seed):
    M = _case(300, 600, 0.1, seed)
    q, scale = _q(300, 600, 0.1, seed, metric)
    for k in KS:
        got = gficf_amd.find_nn_sparse(M, k, metric=metric)
        loose = so.compare(got, _want(q, scale, metric, k), metric)
        print(f"{metric} seed {seed} k {k}: {len(loose)} rows at a near tie of the k-th distance")


def test_k_beyond_the_limits_raises_what_find_nn_raises():
    M = _case(300, 600, 0.1, 1)
    X = np.zeros((600, 3))
    for k, status in ((129, "GFICF_ERR_UNSUPPORTED"), (601, "GFICF_ERR_UNSUPPORTED")):
        with pytest.raises(GficfError) as dense:
            gficf_amd.find_nn(X, k)
        with pytest.raises(GficfError) as sparse:
            gficf_amd.find_nn_sparse(M, k)
        assert sparse.value.status == dense.value.status == status and str(sparse.value) == str(dense.value)
    small = _case(300, 600, 0.1, 1)[:, :20]
    with pytest.raises(GficfError) as dense:
        gficf_amd.find_nn(X[:20], 21)
    with pytest.raises(GficfError) as sparse:
        gficf_amd.find_nn_sparse(small, 21)
    assert sparse.value.status == dense.value.status == "GFICF_ERR_INVALID_ARG" and str(sparse.value) == str(dense.value)


# ------------------------------------------------------------------------------------------------ tile seams
def _seams():
    """{TQ: the largest G that still gets TQ queries per tile}, read off the shape function."""
    top = gficf_amd.find_nn_sparse_shape(1, 300, 16)
    out = {}
    for tq in (8, 4, 2, 1):
        lo, hi = 1, top["max_genes"]                                     # the largest G with tile_queries >= tq
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if gficf_amd.find_nn_sparse_shape(mid, 300, 16)["tile_queries"] >= tq else (lo, mid - 1)
        if gficf_amd.find_nn_sparse_shape(lo, 300, 16)["tile_queries"] == tq:
            out[tq] = lo
    return out, top["max_genes"]


@pytest.mark.parametrize("metric", ("euclidean", "cosine"))
@pytest.mark.parametrize("tq", (8, 4, 2, 1))
def test_tile_seams(tq, metric):
    seams, max_genes = _seams()
    assert set(seams) == {8, 4, 2, 1} and seams[1] == max_genes
    G = seams[tq]
    N = 300 if 300 % tq or tq == 1 else 301                             # not a multiple of the tile
    for g in (G, G + 1):
        if g > max_genes:
            with pytest.raises(GficfError, match=f"GFICF_ERR_UNSUPPORTED.*{max_genes}") as e:
                gficf_amd.find_nn_sparse(so.case(g, N, 40.0 / g, 1), 16, metric=metric)
            assert e.value.status == "GFICF_ERR_UNSUPPORTED"
            with pytest.raises(GficfError):
                gficf_amd.find_nn_sparse_shape(g, N, 16)
            continue
        shape = gficf_amd.find_nn_sparse_shape(g, N, 16)
        assert shape["tile_queries"] == (tq if g == G else tq // 2)
        _check(so.case(g, N, 40.0 / g, 1), metric, 16)
    for n in (tq + 1, 1):                                                # a last tile of one query; a matrix of one cell
        _check(so.case(G, n, 40.0 / G, 2), metric, min(16, n))


# ------------------------------------------------------------------------------------------------ columns
def _columns_matrix():
    """G = 300: ordinary cells, then an empty cell, a cell of one entry, cells one below, at and one above the lane group's
    stride, a cell storing every gene, and a cell with a stored explicit 0."""
    rng = np.random.default_rng(7)
    L = _sparse_knn_lib.LANES
    base = so.case(300, 90, 0.1, 3)
    cols = [(base.indices[base.indptr[c]:base.indptr[c + 1]], base.data[base.indptr[c]:base.indptr[c + 1]]) for c in range(90)]
    for n in (0, 1, L - 1, L, L + 1, 300):
        r = np.sort(rng.choice(300, n, replace=False))
        cols.append((r, rng.gamma(2, 1, n)))
    r = np.sort(rng.choice(300, 20, replace=False))
    v = rng.gamma(2, 1, 20)
    v[5] = 0.0
    cols.append((r, v))
    indptr = np.concatenate([[0], np.cumsum([len(r) for r, _ in cols])])
    M = sp.csc_matrix((np.concatenate([v for _, v in cols]), np.concatenate([r for r, _ in cols]).astype(np.int32), indptr), shape=(300, len(cols)))
    assert M.nnz == indptr[-1] and (M.data == 0).sum() == 1              # the explicit 0 is still stored
    return M


@pytest.mark.parametrize("metric", so.METRICS)
def test_column_lengths(metric):
    M = _columns_matrix()
    got, _ = _check(M, metric, 16)
    if metric in ("cosine", "correlation"):                              # the empty cell: 1 from every other cell, ids ascending
        assert (got["dist"][90, 1:] == 1).all() and list(got["idx"][90]) == [91] + list(range(1, 16))


# ------------------------------------------------------------------------------------------------ ties and duplicates
@pytest.mark.parametrize("metric", so.METRICS)
def test_identical_cells(metric):
    M = sp.lil_matrix(_case(300, 600, 0.1, 2))
    twins = [0, 100, 200, 300]
    for c in twins[1:]:
        M[:, c] = M[:, 0]
    M = sp.csc_matrix(M)
    M.sort_indices()
    got = gficf_amd.find_nn_sparse(M, 16, metric=metric)
    _, scale = so.q_and_scale(M, metric)
    for c in twins:
        assert sorted(got["idx"][c, :4]) == [t + 1 for t in twins]
        d = got["dist"][c, :4]
        assert (np.abs(d * d if metric == "euclidean" else d) <= so.ABS * scale[c, 0]).all()
    assert (np.diff(got["dist"], axis=1) >= 0).all() and (got["dist"][:, 0] == 0).all()
    assert (got["idx"] == np.arange(1, 601)[:, None]).any(axis=1).all()


def test_disjoint_cells_under_cosine():
    N, w, k = 200, 5, 16
    M = sp.csc_matrix((np.random.default_rng(5).gamma(2, 1, N * w), np.arange(N * w, dtype=np.int32), np.arange(0, N * w + 1, w)), shape=(N * w, N))
    got = gficf_amd.find_nn_sparse(M, k, metric="cosine")
    assert (got["dist"][:, 0] == 0).all() and (got["dist"][:, 1:] == 1).all()
    for i in range(N):
        assert list(got["idx"][i]) == [i + 1] + [j + 1 for j in range(N) if j != i][:k - 1]


# ------------------------------------------------------------------------------------------------ slices, ranges, determinism
def _slice_sizes():
    one = 300
    assert gficf_amd.find_nn_sparse_shape(300, one, 16)["slices"] == 1
    many = next(n for n in range(301, 4000, 97) if gficf_amd.find_nn_sparse_shape(300, n, 16)["slices"] > 1)
    return one, many


@pytest.mark.parametrize("which", (0, 1))
def test_slices_and_query_ranges(which):
    N = _slice_sizes()[which]
    shape = gficf_amd.find_nn_sparse_shape(300, N, 16)
    assert (shape["slices"] > 1) == bool(which)
    M = so.case(300, N, 0.1, 3)
    for metric in ("euclidean", "cosine"):
        got, _ = _check(M, metric, 16)
        again = gficf_amd.find_nn_sparse(M, 16, metric=metric)
        assert np.array_equal(got["idx"], again["idx"]) and np.array_equal(got["dist"], again["dist"])
        a = 37
        assert a % shape["tile_queries"]
        parts = [gficf_amd.find_nn_sparse_range(M, 16, b, e, metric) for b, e in ((0, a), (a, N), (0, N), (N, N))]
        assert parts[3]["idx"].shape == (0, 16)
        for key in ("idx", "dist"):
            assert np.array_equal(np.concatenate([parts[0][key], parts[1][key]]), got[key])
            assert np.array_equal(parts[2][key], got[key])


def test_include_self_false_and_the_consumers():
    M = _case(300, 600, 0.1, 1)
    full = gficf_amd.find_nn_sparse(M, 17, metric="cosine")
    got = gficf_amd.find_nn_sparse(M, 16, include_self=False, metric="cosine")
    assert got["idx"].shape == (600, 16) and not (got["idx"] == np.arange(1, 601)[:, None]).any()
    assert np.array_equal(got["idx"], full["idx"][:, 1:]) and np.array_equal(got["dist"], full["dist"][:, 1:])
    edges = gficf_amd.jaccard_edges(full["idx"])
    assert len(edges["from"]) > 0 and np.isfinite(edges["weight"]).all()
    P = gficf_amd.fuzzy_simplicial_set(full["idx"], full["dist"])[0]
    assert P.shape == (600, 600) and (P != P.T).nnz == 0
    eu = gficf_amd.find_nn_sparse(M, 16)
    assert gficf_amd.tsne_affinities(eu["idx"], eu["dist"], 5)[0].shape == (600, 600)


# ------------------------------------------------------------------------------------------------ closed form
@pytest.mark.parametrize("metric", ("euclidean", "cosine"))
def test_ring_closed_form(metric):
    N, w, h = 20000, 32, 15
    got = gficf_amd.find_nn_sparse(ring.ring_matrix(N, w), 2 * h + 1, metric=metric)
    idx, dist = ring.ring_expected(N, w, h, metric)
    assert np.array_equal(got["idx"], idx)
    assert np.array_equal(got["dist"], dist)


# ------------------------------------------------------------------------------------------------ against the dense search
@pytest.mark.parametrize("metric", so.METRICS)
def test_against_the_dense_search(metric):
    """find_nn on the densified cells is the same table in everything but rounding: its f32 chain of 40 terms sets the absolute
    term of rule 3, 40 x 2^-24 of the scale.  find_nn returns no distance beyond its k columns, so the rules run over the ids
    both tables hold (3) and over the ids in which they differ, each table's own q against the dense k-th (4)."""
    G, N, k = 40, 500, 16
    M = so.case(G, N, 0.3, 1)
    got = gficf_amd.find_nn_sparse(M, k, metric=metric)
    ref = gficf_amd.find_nn(np.asarray(M.T.todense()), k, metric=metric)
    _, scale = so.q_and_scale(M, metric)
    abs_term = G * 2.0 ** -24
    sq = (lambda d: d * d) if metric == "euclidean" else (lambda d: d)
    loose = 0
    for i in range(N):
        qg, qr = dict(zip(got["idx"][i], sq(got["dist"][i]))), dict(zip(ref["idx"][i], sq(ref["dist"][i])))
        tol = lambda j, q: so.REL * q + abs_term * scale[i, j - 1]
        for j in set(qg) & set(qr):
            assert abs(qg[j] - qr[j]) <= tol(j, qr[j]), (i, j, qg[j], qr[j])
        if list(got["idx"][i]) != list(ref["idx"][i]):
            kth = sq(ref["dist"][i, k - 1])
            differ = got["idx"][i] != ref["idx"][i]
            for j in set(got["idx"][i][differ]) | set(ref["idx"][i][differ]):
                q = qr[j] if j in qr else qg[j]
                assert abs(q - kth) <= tol(j, kth), (i, j, q, kth)
            loose += 1
    print(f"{metric}: {loose} of {N} rows differ from the dense search at a near tie of the k-th distance")
    assert loose <= 0.01 * N
