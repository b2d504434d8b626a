"""libgficf_sparse_knn.so on the device against the restatement of its contract (tests/helpers/sparse_knn_par.py), bit for bit:
ids by ``np.array_equal``, distances by their bits, no tolerance and no loose rows.  The inputs (tests/helpers/sparse_knn_cases.py)
are long cells around every stride of the tile kernel and amplifier pairs, on which the order of the f64 sums shows in the f32
result (tests/test_sparse_knn_par_cpu.py holds the inputs to that); one case per tile width.

If the pairs alone differ, the kernel's order, tree or fusion is not the header's; if ordinary long cells differ, the loads of
``sk_chain`` or ``sk_load_q`` are wrong."""
import functools

import numpy as np
import pytest

import gficf_amd
from tests.helpers import sparse_knn_cases as sc
from tests.helpers import sparse_knn_oracle as so
from tests.helpers import sparse_knn_par as par

pytestmark = pytest.mark.gpu

TQS = (8, 4, 2, 1)
KS = (16, 65, 128)


def _bits(dist):
    dist = np.ascontiguousarray(dist)
    assert dist.dtype == np.float64
    return dist.view(np.int64)


def _want(G, metric, k, rows=slice(None)):
    idx, dist = par.table(sc.contract(G, metric), k)
    return idx[rows], dist[rows]


def _where_it_differs(got, idx, dist, first_row=0):
    rows = np.flatnonzero((got["idx"] != idx).any(axis=1) | (_bits(got["dist"]) != _bits(dist)).any(axis=1))
    if not len(rows):
        return "equal"
    r = rows[0]
    col = np.flatnonzero((got["idx"][r] != idx[r]) | (_bits(got["dist"][r]) != _bits(dist[r])))[0]
    return (f"{len(rows)} of {len(idx)} rows differ, the first: query {first_row + r} column {col}: id {got['idx'][r, col]} at "
            f"{got['dist'][r, col]!r}, the contract's id {idx[r, col]} at {dist[r, col]!r}; rows {[int(first_row + r) for r in rows[:20]]}")


def _assert_equal(got, idx, dist, first_row=0):
    assert got["idx"].shape == idx.shape and got["idx"].dtype == np.int32
    assert np.array_equal(got["idx"], idx) and np.array_equal(_bits(got["dist"]), _bits(dist)), _where_it_differs(got, idx, dist, first_row)


def _assert_pairs(got, G, metric, k):
    """The mutual distances of the amplifier pairs on their own: a failure here reads as "order", not as "row 37"."""
    c, d = sc.case(G), sc.contract(G, metric)
    lengths = np.diff(c["M"].indptr)
    wrong = []
    for name in ("pairs", "mpairs"):
        for i, j in c[name]:
            for q, cand in ((i, j), (j, i)):
                at = np.flatnonzero(got["idx"][q] == cand + 1)
                assert (par.table(d[q:q + 1], k)[0] == cand + 1).any(), "the cases: a copy is not among its cell's neighbours"
                seen = np.float32(got["dist"][q, at[0]]) if len(at) else None
                if seen is None or seen.view(np.uint32) != d[q, cand].view(np.uint32):
                    wrong.append(f"{name} ({q}, {cand}), {lengths[q]} entries: device {seen!r}, contract {d[q, cand]!r}")
    assert not wrong, (f"{metric}: the summation ORDER (chains, tree or fusion) differs from the header's on {len(wrong)} mutual "
                       f"distances of amplifier pairs: " + "; ".join(wrong[:6]))


# ------------------------------------------------------------------------------------------------ every tile width
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("metric", so.METRICS)
@pytest.mark.parametrize("tq", TQS)
def test_every_tile_width_metric_and_list_length(tq, metric, k):
    G = sc.tile_genes()[tq]
    M = sc.case(G)["M"]
    assert gficf_amd.find_nn_sparse_shape(G, M.shape[1], k)["tile_queries"] == tq
    got = gficf_amd.find_nn_sparse(M, k, metric=metric)
    _assert_pairs(got, G, metric, k)
    _assert_equal(got, *_want(G, metric, k))


@pytest.mark.parametrize("metric", so.METRICS)
@pytest.mark.parametrize("tq", TQS)
def test_ranges_at_every_tile_width(tq, metric):
    """[0, a) and [a, N), a inside an amplifier pair and no multiple of the tile width: the bits of the contract and of [0, N)."""
    G, k = sc.tile_genes()[tq], 16
    c = sc.case(G)
    M, a = c["M"], c["split_at"]
    N = M.shape[1]
    assert (a % tq or tq == 1) and any(i < a <= j for i, j in c["pairs"])
    idx, dist = _want(G, metric, k)
    head = gficf_amd.find_nn_sparse_range(M, k, 0, a, metric)
    tail = gficf_amd.find_nn_sparse_range(M, k, a, N, metric)
    _assert_equal(head, idx[:a], dist[:a])
    _assert_equal(tail, idx[a:], dist[a:], a)
    full = gficf_amd.find_nn_sparse(M, k, metric=metric)
    for key in ("idx", "dist"):
        assert np.array_equal(np.concatenate([head[key], tail[key]]), full[key])


# ------------------------------------------------------------------------------------------------ thirty-two slices
@functools.lru_cache(maxsize=None)
def _many_cells():
    return so.case(300, 8200, 0.1, 5)


@pytest.mark.parametrize("metric", ("euclidean", "manhattan"))
def test_thirty_two_slices_and_both_halves_of_the_list(metric):
    """Five queries against 8 200 cells: one tile, so the candidates are cut into the most slices there are, 32 (31 of
    ceil(8200 / 32) = 257 candidates and a last one of 233; the entries state the slice count only through the workspace, whose
    one piece that grows with the queries holds n_q x slices x k keys of 8 bytes), and k = 128 takes the merge through both
    halves of its list."""
    M, k = _many_cells(), 128
    G, N = M.shape
    wb = gficf_amd.HipOps.sparse_knn_workspace_bytes
    shape = gficf_amd.find_nn_sparse_shape(G, N, k)
    assert shape["tile_queries"] == 8 and shape["slices"] == 1   # all N queries: tiles enough, one slice
    assert wb(G, N, M.nnz, k, 5) - wb(G, N, M.nnz, k, N) == (5 * 32 - N * 1) * k * 8
    for b, e in ((5, 10), (N - 5, N)):
        got = gficf_amd.find_nn_sparse_range(M, k, b, e, metric)
        idx, dist = par.table(par.distance_table(M, metric, b, e), k)
        _assert_equal(got, idx, dist, b)


# ------------------------------------------------------------------------------------------------ the entries
def test_int64_column_pointers_at_the_host_entry():
    G = sc.tile_genes()[8]
    M32 = sc.case(G)["M"]
    M64 = M32.copy()
    M64.indptr, M64.indices = M64.indptr.astype(np.int64), M64.indices.astype(np.int64)
    assert M32.indptr.dtype == np.int32 and M64.indptr.dtype == np.int64
    assert gficf_amd.api._csc_parts(M64)[1].dtype == np.int64 and gficf_amd.api._csc_parts(M32)[1].dtype == np.int32
    for metric in ("euclidean", "correlation"):
        got = gficf_amd.find_nn_sparse(M64, 65, metric=metric)
        narrow = gficf_amd.find_nn_sparse(M32, 65, metric=metric)
        assert np.array_equal(got["idx"], narrow["idx"]) and np.array_equal(_bits(got["dist"]), _bits(narrow["dist"]))
        _assert_equal(got, *_want(G, metric, 65))


def test_a_leading_dimension_beyond_the_queries():
    """The device entry on tables three columns wider than the query range: the same rows, the padding untouched."""
    import torch

    G, k, metric, pad = sc.tile_genes()[4], 65, "cosine", 3
    c = sc.case(G)
    M, a = c["M"], c["split_at"]
    N = M.shape[1]
    ops = gficf_amd.HipOps(0)
    cp, ri, x = (torch.from_numpy(v).to("cuda:0") for v in (M.indptr.astype(np.int64), M.indices.astype(np.int32), M.data))
    ws = torch.empty(ops.sparse_knn_workspace_bytes(G, N, M.nnz, k, N - a), dtype=torch.uint8, device="cuda:0")
    idx = torch.full((k, N - a + pad), -7, dtype=torch.int32, device="cuda:0")
    dist = torch.full((k, N - a + pad), -1.0, dtype=torch.float64, device="cuda:0")
    ops.sparse_knn(G, N, cp, ri, x, k, metric, a, N, ws, idx, dist)
    ops.sparse_knn_sync(ws)
    idx, dist = idx.cpu().numpy().T, dist.cpu().numpy().T
    assert (idx[N - a:] == -7).all() and (dist[N - a:] == -1.0).all()
    _assert_equal({"idx": np.ascontiguousarray(idx[:N - a]), "dist": np.ascontiguousarray(dist[:N - a])}, *_want(G, metric, k, slice(a, N)), a)
