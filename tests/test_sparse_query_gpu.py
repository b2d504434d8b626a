"""libgficf_sparse_query.so on the device against the NumPy oracle of tests/helpers/sparse_query_oracle.py under its rule (rules
1, 3 and 4 of the square search's; no self rule, ids in [1, N]), on small shapes: every metric and list length, every tile-width
seam, the edge sizes, special cells, duplicates, the most slices there are, splits of the queries, the square search's range form
as a second reference, the deferred errors of the QUERY matrix, both column-pointer widths and both distance tables.  Every test
prints the rows that took the rule's second branch (the seeds give 0 on the CPU: tests/test_sparse_query_cpu.py)."""
import numpy as np
import pytest
import scipy.sparse as sp

import gficf_amd
from gficf_amd import GficfError
from tests.helpers import sparse_query_oracle as qo
from tests.helpers import sparse_query_par as qp

pytestmark = pytest.mark.gpu

TINY = 2.0 ** -51


def _bits(dist):
    dist = np.ascontiguousarray(dist)
    assert dist.dtype == np.float64
    return dist.view(np.int64)


def _check(train, Q, k, metric, got=None):
    got = gficf_amd.find_nn_sparse_query(train, Q, k, metric) if got is None else got
    loose = qo.compare(got, qo.oracle(train, Q, metric, k), metric)
    print(f"{metric} G {train.shape[0]} N {train.shape[1]} M {Q.shape[1]} k {k}: {len(loose)} rows in the second branch of rule 4")
    return got


def _same(a, b):
    return np.array_equal(a["idx"], b["idx"]) and np.array_equal(_bits(a["dist"]), _bits(b["dist"]))


# ------------------------------------------------------------------------------------------------ metrics and list lengths
@pytest.fixture(scope="module")
def basic():
    G, N, M, lo, hi, seed = qo.BASIC
    return qo.pair_case(G, N, M, lo, hi, seed)


@pytest.mark.parametrize("k", qo.BASIC_KS)
@pytest.mark.parametrize("metric", qo.METRICS)
def test_every_metric_and_list_length(basic, metric, k):
    train, Q = basic
    got = _check(train, Q, k, metric)
    assert got["idx"].shape == (37, k) and got["idx"].flags.c_contiguous and got["dist"].flags.c_contiguous


# ------------------------------------------------------------------------------------------------ tile-width seams
def _seams():
    """The largest G of every tile width and one past it, found from the shape entry."""
    tq_of = lambda G: gficf_amd.find_nn_sparse_query_shape(G, qo.SEAM_N, 3, qo.SEAM_K)["tile_queries"]
    top = gficf_amd.find_nn_sparse_query_shape(1, qo.SEAM_N, 3, qo.SEAM_K)["max_genes"]
    out = []
    for tq in (8, 4, 2):
        lo, hi = 1, top                                        # the largest G with tile_queries >= tq
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if tq_of(mid) >= tq else (lo, mid - 1)
        out += [lo, lo + 1]
    return tuple(out + [top])


def test_the_seams_are_where_the_cases_are():
    assert _seams() == qo.SEAM_GS


@pytest.mark.parametrize("G", qo.SEAM_GS)
def test_tile_width_seams(G):
    tq = gficf_amd.find_nn_sparse_query_shape(G, qo.SEAM_N, 3, qo.SEAM_K)["tile_queries"]
    for M in sorted({1, tq - 1, tq, tq + 1} - {0}):
        train, Q = qo.seam_case(G, M)
        assert train.indices.min() == 0 and train.indices.max() == G - 1 and Q.indices.max() == G - 1
        for metric in ("euclidean", "cosine"):
            _check(train, Q, qo.SEAM_K, metric)


def test_more_genes_than_lds_holds_are_unsupported():
    train, Q = qo.seam_case(32769, 2)
    with pytest.raises(GficfError) as e:
        gficf_amd.find_nn_sparse_query(train, Q, 5)
    assert e.value.status == "GFICF_ERR_UNSUPPORTED" and "32768" in str(e.value)


# ------------------------------------------------------------------------------------------------ limits and edge sizes
def test_limits_of_k(basic):
    train, Q = basic
    with pytest.raises(GficfError) as e:
        gficf_amd.find_nn_sparse_query(train, Q, 129)
    assert e.value.status == "GFICF_ERR_UNSUPPORTED"
    few = sp.csc_matrix(train[:, :20])
    with pytest.raises(GficfError) as e:
        gficf_amd.find_nn_sparse_query(few, Q, 21)
    assert e.value.status == "GFICF_ERR_INVALID_ARG"
    got = _check(few, Q, 20, "manhattan")                      # k = N: every training cell, once
    assert (np.sort(got["idx"], axis=1) == np.arange(1, 21)).all()
    one = sp.csc_matrix(train[:, :1])
    got = _check(one, Q, 1, "euclidean")                       # N = k = 1
    assert (got["idx"] == 1).all()
    none = gficf_amd.find_nn_sparse_query(train, sp.csc_matrix((300, 0)), 7)                  # M = 0: empty tables, no error
    assert none["idx"].shape == (0, 7) and none["idx"].dtype == np.int32 and none["dist"].shape == (0, 7) and none["dist"].dtype == np.float64
    assert _same(gficf_amd.find_nn_sparse_query(train, Q, 16), gficf_amd.find_nn_sparse_query(train, Q, 16))   # and the context is fine


# ------------------------------------------------------------------------------------------------ special cells
def test_special_cells(basic):
    train, Q = basic
    G, N = train.shape
    empty = sp.csc_matrix((G, 1))
    # an empty query
    Qe = sp.hstack([Q[:, :5], empty, Q[:, 5:9]], format="csc")
    got = _check(train, Qe, 16, "cosine")
    assert (got["dist"][5] == 1).all() and np.array_equal(got["idx"][5], np.arange(1, 17))
    got = _check(train, Qe, 16, "correlation")
    assert (got["dist"][5] == 1).all() and np.array_equal(got["idx"][5], np.arange(1, 17))
    got = _check(train, Qe, 128, "euclidean")
    nb = np.asarray(train.astype(np.float32).astype(np.float64).power(2).sum(axis=0)).ravel()
    want = np.sqrt(nb)[got["idx"][5] - 1]
    assert np.abs(got["dist"][5] / want - 1).max() <= 2.0 ** -23
    got = _check(train, Qe, 16, "manhattan")
    # an empty training cell
    te = sp.hstack([train[:, :7], empty, train[:, 7:60]], format="csc")
    for metric in qo.METRICS:
        got = _check(te, Q, 61, metric)                        # k = N: the empty cell is in every row
        assert ((got["idx"] == 8).sum(axis=1) == 1).all()
        if metric in ("cosine", "correlation"):
            assert (got["dist"][got["idx"] == 8] == 1).all()
    # queries storing genes no training cell stores: 40 more genes, stored by the queries alone
    wide_t = sp.vstack([train, sp.csc_matrix((40, N))], format="csc")
    extra = sp.random(40, Q.shape[1], 0.3, random_state=np.random.default_rng(3), format="csc")
    wide_q = sp.vstack([Q, extra], format="csc")
    wide_q.sort_indices()
    for metric in qo.METRICS:
        _check(wide_t, wide_q, 16, metric)
    # a stored 0
    Qz = Q.copy()
    Qz.data[Qz.indptr[2]] = 0.0
    tz = train.copy()
    tz.data[tz.indptr[3] + 1] = 0.0
    for metric in qo.METRICS:
        _check(tz, Qz, 16, metric)


def test_duplicate_training_cells_and_a_query_equal_to_them(basic):
    train, Q = basic
    cell = train[:, 11]
    dup = sp.hstack([train[:, :30], cell, train[:, 30:90], cell, train[:, 90:]], format="csc")    # ids 12, 31 and 92 are one cell
    Qd = sp.hstack([Q[:, :3], cell, Q[:, 3:]], format="csc")
    for metric in qo.METRICS:
        # the reference is the restated contract, bit for bit: equal cells are equal arithmetic there, as on the device, while the
        # oracle's own summation may order the three copies by its noise
        got = gficf_amd.find_nn_sparse_query(dup, Qd, 16, metric)
        idx, dist = qp.table(qp.distance_table(dup, Qd, metric), 16)
        assert np.array_equal(got["idx"], idx) and np.array_equal(_bits(got["dist"]), _bits(dist)), metric
        ids, d = got["idx"][3, :3], got["dist"][3, :3]
        assert sorted(ids) == [12, 31, 92], (metric, ids)
        if metric in ("euclidean", "manhattan"):
            assert (d == 0).all() and list(ids) == [12, 31, 92]                                    # exactly 0, ids ascending
        else:
            assert (d >= 0).all() and (d <= TINY).all()
            assert len(set(d)) == 1 and list(ids) == [12, 31, 92]                                  # one cell, one arithmetic: the id decides


# ------------------------------------------------------------------------------------------------ thirty-two slices
def test_thirty_two_slices():
    """Five queries against 8 200 training cells: one tile, so the candidates are cut into the most slices there are, 32: 31 of
    ceil(8200 / 32) = 257 and a last one of 233.  k = 128 takes the merge through both halves of its list.  The reference here
    is the restated contract, bit for bit (the oracle would densify 8 205 x 8 205 pairs)."""
    from tests.helpers import sparse_knn_oracle as so

    A = so.case(300, 8205, 0.1, 5)
    train, Q = sp.csc_matrix(A[:, :8200]), sp.csc_matrix(A[:, 8200:])
    shape = gficf_amd.find_nn_sparse_query_shape(300, 8200, 5, 128)
    assert shape == {"tile_queries": 8, "slices": 32, "max_genes": 32768}
    assert -(-8200 // 32) == 257 and 8200 - 31 * 257 == 233
    assert gficf_amd.HipOps.sparse_query_workspace_bytes(300, 8200, train.nnz, 5, Q.nnz, 128) >= 5 * 32 * 128 * 8 + 4 * (train.nnz + Q.nnz)
    for metric in ("euclidean", "manhattan"):
        got = gficf_amd.find_nn_sparse_query(train, Q, 128, metric)
        idx, dist = qp.table(qp.distance_table(train, Q, metric), 128)
        assert np.array_equal(got["idx"], idx) and np.array_equal(_bits(got["dist"]), _bits(dist)), metric
        assert (got["idx"].max(axis=1) > 8200 - 233).any() and (got["idx"].min(axis=1) <= 257).any()   # the first and the last slice are heard


# ------------------------------------------------------------------------------------------------ splits of the queries
def _device_call(train, Q, k, metric, pad=0, want32=False):
    import torch

    dev = "cuda:0"
    ops = gficf_amd.HipOps(0)
    G, N = train.shape
    M = Q.shape[1]
    t = [torch.from_numpy(v).to(dev) for v in (train.indptr.astype(np.int64), train.indices.astype(np.int32), train.data.astype(np.float64))]
    q = [torch.from_numpy(v).to(dev) for v in (Q.indptr.astype(np.int64), Q.indices.astype(np.int32), Q.data.astype(np.float64))]
    ws = torch.empty(ops.sparse_query_workspace_bytes(G, N, train.nnz, M, Q.nnz, k), dtype=torch.uint8, device=dev)
    idx = torch.full((k, M + pad), -7, dtype=torch.int32, device=dev)
    dist = torch.full((k, M + pad), -1.0, dtype=torch.float64, device=dev)
    dist32 = torch.full((k, M + pad), -1.0, dtype=torch.float32, device=dev) if want32 else None
    ops.sparse_query(G, N, *t, M, *q, k, metric, ws, idx, dist, dist32)
    ops.sparse_query_sync(ws)
    out = {"idx": idx.cpu().numpy().T, "dist": dist.cpu().numpy().T}
    if want32:
        out["dist32"] = dist32.cpu().numpy().T
    return out


@pytest.mark.parametrize("metric", qo.METRICS)
def test_two_parts_of_the_queries_give_the_bits_of_the_whole(basic, metric):
    train, Q = basic
    a, k, pad = 13, 16, 3
    whole = _check(train, Q, k, metric)
    head, tail = (gficf_amd.find_nn_sparse_query(train, sp.csc_matrix(part), k, metric) for part in (Q[:, :a], Q[:, a:]))
    assert _same({key: np.concatenate([head[key], tail[key]]) for key in ("idx", "dist")}, whole)
    parts = [_device_call(train, sp.csc_matrix(part), k, metric, pad) for part in (Q[:, :a], Q[:, a:])]
    for part, rows in zip(parts, (slice(0, a), slice(a, 37))):
        n = rows.stop - rows.start
        assert (part["idx"][n:] == -7).all() and (part["dist"][n:] == -1.0).all()              # the padding is untouched
        assert np.array_equal(part["idx"][:n], whole["idx"][rows]) and np.array_equal(_bits(part["dist"][:n]), _bits(whole["dist"][rows]))


# ------------------------------------------------------------------------------------------------ the square search's range form
@pytest.mark.parametrize("metric", qo.METRICS)
def test_against_the_range_form_of_the_square_search(metric):
    """find_nn_sparse_query(A, A[:, a:b]) streams what find_nn_sparse_range(A, k, a, b) streams: the same table, but for the self
    entry, which the square search writes as 0 without arithmetic and this one computes."""
    A = qo.cells(300, 187, 12, 40, 5)
    a, b, k = 50, 91, 16
    sq = gficf_amd.find_nn_sparse_range(A, k, a, b, metric)
    got = gficf_amd.find_nn_sparse_query(A, sp.csc_matrix(A[:, a:b]), k, metric)
    own = np.arange(a + 1, b + 1)
    assert np.array_equal(sq["idx"][:, 0], own) and (sq["dist"][:, 0] == 0).all()
    if metric in ("euclidean", "manhattan"):
        assert _same(got, sq)
    else:
        assert np.array_equal(got["idx"], sq["idx"])
        assert np.array_equal(_bits(got["dist"][:, 1:]), _bits(sq["dist"][:, 1:]))
        assert (got["dist"][:, 0] >= 0).all() and (got["dist"][:, 0] <= TINY).all()
        print(f"{metric}: {(got['dist'][:, 0] > 0).sum()} of {b - a} self entries are not 0")


# ------------------------------------------------------------------------------------------------ deferred errors of the query matrix
def test_deferred_errors_of_the_query_matrix(basic):
    train, Q = basic
    k = 8
    b = Q.indptr[4]
    swapped = Q.copy()
    swapped.indices[b], swapped.indices[b + 1] = Q.indices[b + 1], Q.indices[b]                 # rows descending within a column
    beyond = Q.copy()
    beyond.indices[Q.indptr[5] - 1] = 300                                                      # a row id = G
    nan = Q.copy()
    nan.data[b + 2] = np.nan
    for bad, status in ((swapped, "GFICF_ERR_BAD_CSC"), (beyond, "GFICF_ERR_BAD_CSC"), (nan, "GFICF_ERR_BAD_VALUE")):
        with pytest.raises(GficfError) as e:
            _device_call(train, bad, k, "euclidean")
        assert e.value.status == status
        again = _device_call(train, Q, k, "euclidean")                                         # the context is usable afterwards
        _check(train, Q, k, "euclidean", {key: np.ascontiguousarray(again[key]) for key in ("idx", "dist")})
    with pytest.raises(GficfError) as e:                                                       # and the training matrix's, through the same word
        _device_call(nan, Q, k, "euclidean")
    assert e.value.status == "GFICF_ERR_BAD_VALUE"


# ------------------------------------------------------------------------------------------------ the entries
def test_int64_column_pointers_for_either_matrix(basic):
    train, Q = basic
    want = gficf_amd.find_nn_sparse_query(train, Q, 65, "correlation")
    assert train.indptr.dtype == np.int32 and Q.indptr.dtype == np.int32
    for wide_t, wide_q in ((True, False), (False, True), (True, True)):
        t, q = train.copy(), Q.copy()
        if wide_t:
            t.indptr, t.indices = t.indptr.astype(np.int64), t.indices.astype(np.int64)
        if wide_q:
            q.indptr, q.indices = q.indptr.astype(np.int64), q.indices.astype(np.int64)
        assert gficf_amd.api._csc_parts(t)[1].dtype == (np.int64 if wide_t else np.int32)
        assert gficf_amd.api._csc_parts(q)[1].dtype == (np.int64 if wide_q else np.int32)
        assert _same(gficf_amd.find_nn_sparse_query(t, q, 65, "correlation"), want)
    _check(train, Q, 65, "correlation", want)


@pytest.mark.parametrize("metric", qo.METRICS)
def test_the_f32_table_is_the_f64_one_cast(basic, metric):
    train, Q = basic
    got = _device_call(train, Q, 65, metric, want32=True)
    assert got["dist32"].dtype == np.float32 and np.array_equal(got["dist32"].astype(np.float64), got["dist"])
    assert np.array_equal(got["dist32"].view(np.uint32), got["dist"].astype(np.float32).view(np.uint32))
    assert _same({key: np.ascontiguousarray(got[key]) for key in ("idx", "dist")}, gficf_amd.find_nn_sparse_query(train, Q, 65, metric))
