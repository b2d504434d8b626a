"""libgficf_sparse_query.so on the device against the restatement of its contract (tests/helpers/sparse_query_par.py: the square
search's restatement on the stacked matrix, no new arithmetic), bit for bit: ids by ``np.array_equal``, distances by their bits,
no tolerance and no loose rows.  The inputs are the amplifier cases of tests/helpers/sparse_knn_cases.py split into training
cells and queries (``sparse_query_par.split``): the second member of every amplifier and manhattan pair is a query, its twin
stays; a dozen long cells return as exact duplicates; so does the empty cell.  tests/test_sparse_query_cpu.py holds the inputs
to showing every wrong summation order in at least three query -> twin distances at every (metric, tile width).

If the twins alone differ, the kernel's order, tree or fusion is not the header's; if ordinary long cells differ, the loads of
``sk_chain`` or ``sk_load_q``, or the scatter of the queries from the second matrix, are wrong."""
import numpy as np
import pytest

import gficf_amd
from tests.helpers import sparse_knn_cases as sc
from tests.helpers import sparse_query_par as qp

pytestmark = pytest.mark.gpu

TQS = (8, 4, 2, 1)
KS = (16, 65, 128)


def _bits(dist):
    dist = np.ascontiguousarray(dist)
    assert dist.dtype == np.float64
    return dist.view(np.int64)


def _where_it_differs(got, idx, dist):
    rows = np.flatnonzero((got["idx"] != idx).any(axis=1) | (_bits(got["dist"]) != _bits(dist)).any(axis=1))
    if not len(rows):
        return "equal"
    r = rows[0]
    col = np.flatnonzero((got["idx"][r] != idx[r]) | (_bits(got["dist"][r]) != _bits(dist[r])))[0]
    return (f"{len(rows)} of {len(idx)} rows differ, the first: query {r} column {col}: id {got['idx'][r, col]} at "
            f"{got['dist'][r, col]!r}, the contract's id {idx[r, col]} at {dist[r, col]!r}; rows {[int(r) for r in rows[:20]]}")


def _assert_twins(got, G, metric, k):
    """The query -> twin distances on their own: a failure here reads as "order", not as "row 37"."""
    s, d = qp.split(G), qp.contract(G, metric)
    lengths = np.diff(s["Q"].indptr)
    wrong = []
    for name in ("twins", "mtwins"):
        for q, t in s[name]:
            assert (qp.table(d[q:q + 1], k)[0] == t + 1).any(), "the cases: a twin is not among its query's neighbours"
            at = np.flatnonzero(got["idx"][q] == t + 1)
            seen = np.float32(got["dist"][q, at[0]]) if len(at) else None
            if seen is None or seen.view(np.uint32) != d[q, t].view(np.uint32):
                wrong.append(f"{name} (query {q}, training cell {t}), {lengths[q]} entries: device {seen!r}, contract {d[q, t]!r}")
    assert not wrong, (f"{metric}: the summation ORDER (chains, tree or fusion) differs from the header's on {len(wrong)} query -> twin "
                       f"distances: " + "; ".join(wrong[:6]))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("metric", qp.METRICS)
@pytest.mark.parametrize("tq", TQS)
def test_every_tile_width_metric_and_list_length(tq, metric, k):
    G = sc.tile_genes()[tq]
    s = qp.split(G)
    train, Q = s["train"], s["Q"]
    assert gficf_amd.find_nn_sparse_query_shape(G, train.shape[1], Q.shape[1], k)["tile_queries"] == tq and Q.shape[1] % 2
    got = gficf_amd.find_nn_sparse_query(train, Q, k, metric)
    _assert_twins(got, G, metric, k)
    idx, dist = qp.table(qp.contract(G, metric), k)
    assert got["idx"].shape == idx.shape and got["idx"].dtype == np.int32
    assert np.array_equal(got["idx"], idx) and np.array_equal(_bits(got["dist"]), _bits(dist)), _where_it_differs(got, idx, dist)
    for q, t in s["duplicates"]:                                # a query equal to a training cell, as the header says
        if q == s["empty"]:
            continue
        own = got["dist"][q][got["idx"][q] == t + 1]
        assert len(own) == 1 and (own[0] == 0 if metric in ("euclidean", "manhattan") else 0 <= own[0] <= 2.0 ** -51), (q, t, own)
