"""GPU: libgficf_umap.so (fuzzy graph, layout, the chained embedding) and its Python mirror.

Graph.  Checked against its defining properties in f64 from the device's own sigma, rho and memberships
(tests/helpers/umap_cases.check_graph): no second implementation in the loop.

Layout against the port, the same P and initial coordinates given to both.  The yardstick is the numpy port of
tests/helpers/umap_np.py run in f64.  On every case the port was also run in f32 on the CPU and the largest coordinate deviation
between its two runs recorded: MEASURED below (``python -m tests.helpers.umap_cases`` prints the table).  That deviation is the
size of a legitimate difference between two correct evaluations of different precision; the test constant is 8 x it, never
below 64 * 2^-24 * 10 (64 f32 roundings at the largest coordinate).  No vertex is excluded.  In epoch 0 no entry is due (the
schedule word is below 2^32), so the cases over [0, 1) also assert that the coordinates come back untouched.

The hub graph.  The 2 000 points of the unit sphere in 10-D do not have the origin as their nearest neighbour (about 117 of
them lie within 60 degrees of any one, hence closer to it than the origin; see umap_cases.hub_table), so the exact table is
amended as an approximate search might return it: every row's last column names the origin.  The shape and what it is for
are unchanged: 2 001 points, one row of P with 2 000 entries, the long-row paths of symmetrisation and layout.

Quality.  Trustworthiness and 15-NN label purity of full runs against the port's own figures over the same seeds
(MEASURED_QUALITY, recomputed with the committed port by the same command); the untouched initial plane has 0.909 / 0.819."""
import numpy as np
import pytest
import scipy.sparse as sp

import gficf_amd
from gficf_amd import GficfError, synth
from gficf_amd.api import HipOps
from tests.helpers import umap_cases as uc
from tests.helpers import umap_np as un

pytestmark = pytest.mark.gpu

# |port f32 - port f64|, largest coordinate, per layout case (graph, curve, epochs of 200)
MEASURED = {
    ("rand", "tumap", "0-1"): 4.736e-07,
    ("rand", "tumap", "100-101"): 5.424e-05,
    ("rand", "tumap", "0-3"): 6.416e-03,
    ("rand", "umap", "0-1"): 4.736e-07,
    ("rand", "umap", "100-101"): 1.100e-04,
    ("rand", "umap", "0-3"): 1.195e-02,
    ("hub", "tumap", "0-1"): 4.697e-07,
    ("hub", "tumap", "100-101"): 4.367e-04,
    ("hub", "tumap", "0-3"): 2.888e-03,
    ("hub", "umap", "0-1"): 4.697e-07,
    ("hub", "umap", "100-101"): 5.780e-05,
    ("hub", "umap", "0-3"): 7.789e-03,
    ("crafted", "tumap", "100-101"): 2.770e-04,
}
# (trustworthiness, purity) of the port, seeds 1 - 5, 200 epochs, 1 200 x 20 blobs
MEASURED_QUALITY = {
    "tumap": [(0.97842, 1.0), (0.97885, 1.0), (0.97805, 1.0), (0.97880, 1.0), (0.97801, 1.0)],
    "umap": [(0.97718, 1.0), (0.97746, 1.0), (0.97791, 1.0), (0.97773, 1.0), (0.97755, 1.0)],
}


def _nn(X, k):
    r = gficf_amd.find_nn(X, k, True, "euclidean")
    return r["idx"], r["dist"]


def _graph(idx, dist, mix=1.0, lc=1.0):
    P, sigma, rho, W = gficf_amd.fuzzy_simplicial_set(idx, dist, mix, lc, ret_memberships=True)
    uc.check_graph(idx, dist, P, sigma, rho, W, mix=mix, lc=lc)
    return P, sigma, rho, W


def _same_bits(A, B):
    return (np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
            and np.array_equal(A.data.view(np.uint32), B.data.view(np.uint32)))


# ------------------------------------------------------------------------------------------------ graph
@pytest.fixture(scope="module")
def graph_x():
    return uc.graph_input()


@pytest.mark.parametrize("k", uc.GRAPH_KS)
def test_graph_properties(graph_x, k):
    idx, dist = _nn(graph_x, k)
    P, sigma, rho, W = _graph(idx, dist)
    assert (dist[uc.GRAPH_CENTRE, 1:] == dist[uc.GRAPH_CENTRE, 1]).all()            # the row of one distance
    if k <= 20:
        assert (rho[uc.GRAPH_BLOCK] == 0).all()                                      # the identical points
    if 3 <= k <= 20:                                                                 # k - 1 ones exceed log2(k): the global-mean floor
        assert np.allclose(sigma[uc.GRAPH_BLOCK], 1e-3 * dist.mean(), rtol=1e-5)
    P2, sigma2, rho2, W2 = gficf_amd.fuzzy_simplicial_set(idx, dist, ret_memberships=True)
    assert _same_bits(P, P2) and np.array_equal(sigma, sigma2) and np.array_equal(rho, rho2) and np.array_equal(W, W2)


@pytest.mark.parametrize("mix,lc", [(0.0, 1.0), (0.5, 1.0), (1.0, 1.5), (1.0, 2.0)])
def test_graph_mix_ratio_and_local_connectivity(graph_x, mix, lc):
    idx, dist = _nn(graph_x, 15)
    P, _, _, _ = _graph(idx, dist, mix, lc)
    if mix == 0.0:                                                                   # the intersection: mutual neighbours only
        assert P.nnz < gficf_amd.fuzzy_simplicial_set(idx, dist)[0].nnz


@pytest.fixture(scope="module")
def hub_nn():
    return uc.hub_table(*_nn(uc.hub_points(), 15))


def test_graph_hub(hub_nn):
    idx, dist = hub_nn
    P, _, _, _ = _graph(idx, dist)
    assert np.diff(P.indptr).max() == 2000 and np.diff(P.indptr)[2000] == 2000      # the origin's row names every other point


def test_graph_deferred_errors(graph_x):
    idx, dist = _nn(graph_x, 5)
    bad = idx.copy()
    bad[7, 2] = 301
    with pytest.raises(GficfError) as e:
        gficf_amd.fuzzy_simplicial_set(bad, dist)
    assert e.value.status == "GFICF_ERR_BAD_ID"
    bad[7, 2] = 0
    with pytest.raises(GficfError) as e:
        gficf_amd.fuzzy_simplicial_set(bad, dist)
    assert e.value.status == "GFICF_ERR_BAD_ID"
    for v in (np.nan, np.inf):
        d = dist.copy()
        d[9, 3] = v
        with pytest.raises(GficfError) as e:
            gficf_amd.fuzzy_simplicial_set(idx, d)
        assert e.value.status == "GFICF_ERR_BAD_VALUE"
    d = dist.copy()
    d[:, 0] = -1e-7                                                                  # what 1 - cos rounds to: taken as 0
    assert _same_bits(gficf_amd.fuzzy_simplicial_set(idx, d)[0], gficf_amd.fuzzy_simplicial_set(idx, dist)[0])
    with pytest.raises(GficfError) as e:
        gficf_amd.fuzzy_simplicial_set(idx[:, :1], dist[:, :1])
    assert e.value.status == "GFICF_ERR_INVALID_ARG"


# ------------------------------------------------------------------------------------------------ layout against the port
def _device_layout(name, ab, rng_name, **kw):
    P, Y0 = uc.crafted() if name == "crafted" else uc.layout_graph(name)
    a, b = uc.AB[ab]
    lo, hi = uc.RANGES[rng_name]
    return gficf_amd.umap_layout(P, Y0, uc.LAYOUT_EPOCHS, a, b, seed=uc.LAYOUT_SEED, epoch_begin=lo, epoch_end=hi, **kw), Y0


@pytest.mark.parametrize("case", uc.layout_cases(), ids=lambda c: "-".join(c))
def test_layout_against_port(case):
    got, Y0 = _device_layout(*case)
    want = uc.port_layout(*case, np.float64)
    err = float(np.abs(got.astype(np.float64) - want).max())
    tol = uc.tolerance(MEASURED[case])
    print(f"{case}: |device - port f64| = {err:.3e}, port f32 / f64 = {MEASURED[case]:.3e}, tolerance {tol:.3e}")
    assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all()
    assert err <= tol
    if case[2] == "0-1":
        assert np.array_equal(got, Y0.astype(np.float32))                           # no entry is due in epoch 0
    else:
        assert np.abs(want - Y0).max() > 10 * tol                                    # the sweep is far above what the tolerance forgives


def test_layout_crafted_case_takes_the_zero_distance_branches():
    P, Y0 = uc.crafted()
    assert len(np.unique(Y0[100:150], axis=0)) == 1
    q = un.schedule(P.data)
    fire = un.due(q, 100)
    rows = np.repeat(np.arange(P.shape[0]), np.diff(P.indptr))
    inside = (rows >= 100) & (rows < 150) & (P.indices >= 100) & (P.indices < 150) & fire
    assert inside.any()                                                              # an attraction at d2 == 0 happens in that epoch


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("name,ab", [("rand", "tumap"), ("rand", "umap"), ("hub", "tumap")])
def test_layout_same_bits_and_split_equals_whole(name, ab):
    P, Y0 = uc.layout_graph(name)
    a, b = uc.AB[ab]
    whole = gficf_amd.umap_layout(P, Y0, 200, a, b, seed=7)
    assert np.array_equal(gficf_amd.umap_layout(P, Y0, 200, a, b, seed=7), whole)
    first = gficf_amd.umap_layout(P, Y0, 200, a, b, seed=7, epoch_begin=0, epoch_end=100)
    assert np.array_equal(gficf_amd.umap_layout(P, first, 200, a, b, seed=7, epoch_begin=100, epoch_end=200), whole)
    odd = gficf_amd.umap_layout(P, Y0, 200, a, b, seed=7, epoch_begin=0, epoch_end=33)           # an odd count ends in the second buffer
    assert np.array_equal(gficf_amd.umap_layout(P, odd, 200, a, b, seed=7, epoch_begin=33, epoch_end=200), whole)
    assert not np.array_equal(gficf_amd.umap_layout(P, Y0, 200, a, b, seed=8), whole)
    assert np.isfinite(whole).all()


def test_layout_many_negative_samples_and_none():
    P, Y0 = uc.layout_graph("rand")
    for rate in (0, 1, 8, 9, 20):                                                    # fewer than, as many as and more than the lanes of a group
        got = gficf_amd.umap_layout(P, Y0, 200, negative_sample_rate=rate, seed=3, epoch_begin=100, epoch_end=102)
        want = un.layout(P, Y0, 200, negative_sample_rate=rate, seed=3, epoch_begin=100, epoch_end=102, dtype=np.float64)
        f32 = un.layout(P, Y0, 200, negative_sample_rate=rate, seed=3, epoch_begin=100, epoch_end=102, dtype=np.float32)
        tol = uc.tolerance(float(np.abs(f32 - want).max()))
        assert np.abs(got - want).max() <= tol, rate


def test_chain_equals_its_stages():
    """gficf_umap_host against find_nn -> fuzzy_simplicial_set -> umap_layout, bit for bit, and the device-resident chain of
    HipOps (the graph reads the search's own output, no copy or conversion in between)."""
    X = uc.random_input()
    Y0 = uc.plane_init(X)
    r = gficf_amd.umap(X, Y0, n_neighbors=15, n_epochs=50, a=1.8956, b=0.8006, seed=5)
    idx, dist = _nn(X, 15)
    assert np.array_equal(r["nn"]["idx"], idx) and np.array_equal(r["nn"]["dist"], dist)
    P = gficf_amd.fuzzy_simplicial_set(idx, dist)[0]
    assert _same_bits(sp.csr_matrix(r["graph"]), P)
    Y = gficf_amd.umap_layout(P, Y0, 50, 1.8956, 0.8006, seed=5)
    assert np.array_equal(r["embedding"], Y.astype(np.float64))
    assert r["n_epochs"] == 50 and r["n_neighbors"] == 15 and r["metric"] == "euclidean"

    import torch

    ops = HipOps(0)
    N, d, k = X.shape[0], X.shape[1], 15
    dev = "cuda:0"
    X_cm = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev)
    pts = torch.zeros((N, ops.knn_dpad(d)), dtype=torch.float32, device=dev)
    ops.knn_prepare(X_cm, N, d, "euclidean", pts)
    kws = torch.empty(ops.knn_workspace_bytes(N, N, k), dtype=torch.uint8, device=dev)
    d_idx = torch.empty((k, N), dtype=torch.int32, device=dev)
    d_dist = torch.empty((k, N), dtype=torch.float32, device=dev)
    ops.knn_search(pts, N, d, k, "euclidean", 0, N, kws, d_idx, d_dist)
    cap = 2 * N * k
    gws = torch.empty(ops.umap_graph_workspace_bytes(N, k), dtype=torch.uint8, device=dev)
    rowptr = torch.empty(N + 1, dtype=torch.int64, device=dev)
    col = torch.empty(cap, dtype=torch.int32, device=dev)
    val = torch.empty(cap, dtype=torch.float32, device=dev)
    nnz = torch.zeros(1, dtype=torch.int64, device=dev)
    ops.umap_graph(d_idx, d_dist, N, k, gws, rowptr, col, val, nnz)
    lws = torch.empty(ops.umap_layout_workspace_bytes(N, cap), dtype=torch.uint8, device=dev)
    d_Y = torch.from_numpy(Y0.astype(np.float32)).to(dev)
    ops.umap_layout(N, rowptr, col, val, cap, 1.8956, 0.8006, 1.0, 1.0, 5, 50, 0, 50, 5, d_Y, lws)
    ops.umap_sync(gws)
    ops.umap_sync(lws)
    assert int(nnz.item()) == P.nnz
    assert np.array_equal(d_Y.cpu().numpy(), Y)


def _pca_data(cells):
    return {"pca": {"cells": cells}}


def test_run_reduction_is_a_function_of_its_seed():
    _, _, cells = uc.quality_input()
    a = gficf_amd.runReduction(_pca_data(cells), seed=3, n_epochs=60, verbose=False)
    b = gficf_amd.runReduction(_pca_data(cells), seed=3, n_epochs=60, verbose=False)
    c = gficf_amd.runReduction(_pca_data(cells), seed=4, n_epochs=60, verbose=False)
    assert list(a["embedded"].columns) == ["X", "Y"] and a["embedded"].shape == (1200, 2)
    assert a["embedded"].equals(b["embedded"]) and not a["embedded"].equals(c["embedded"])
    assert a["reduction"] == "tumap" and a["uwot"]["a"] == 1.0 and a["uwot"]["b"] == 1.0 and a["uwot"]["seed"] == 3
    assert set(a["uwot"]) == {"embedding", "graph", "nn", "a", "b", "n_neighbors", "metric", "n_epochs", "seed"}
    assert a["uwot"]["graph"].shape == (1200, 1200) and a["uwot"]["nn"]["idx"].shape == (1200, 15)
    d = gficf_amd.runReduction(_pca_data(cells), seed=3, n_epochs=60, ret_model_pred=False, verbose=False)
    assert "uwot" not in d and d["embedded"].equals(a["embedded"])


# ------------------------------------------------------------------------------------------------ quality, full run
@pytest.mark.parametrize("reduction", ["tumap", "umap"])
def test_quality_of_full_runs(reduction):
    X, labels, cells = uc.quality_input()
    port_trust = min(t for t, _ in MEASURED_QUALITY[reduction])
    for seed in uc.QUALITY_SEEDS:
        data = gficf_amd.runReduction(_pca_data(cells), reduction=reduction, seed=seed, n_epochs=uc.QUALITY_EPOCHS, verbose=False)
        Y = np.asarray(data["embedded"])
        assert np.isfinite(Y).all()
        trust, purity = un.quality(X, Y, labels)
        print(f"{reduction} seed {seed}: trustworthiness {trust:.5f} (port at least {port_trust:.5f}), purity {purity:.4f}")
        assert trust >= port_trust - 0.01
        assert purity >= 0.99
    if reduction == "umap":
        assert abs(data["uwot"]["a"] - 1.8956) < 1e-3 and abs(data["uwot"]["b"] - 0.8006) < 1e-3


# ------------------------------------------------------------------------------------------------ end to end
def test_pipeline_end_to_end():
    colptr, rowidx, x = synth.counts_csc(1500, 800)
    M = sp.csc_matrix((x, rowidx, colptr), shape=(1500, 800))
    data = gficf_amd.gficf(M, normalize=False, verbose=False)
    data = gficf_amd.runPCA(data, dim=10)
    data = gficf_amd.runReduction(data, verbose=False)
    emb = np.asarray(data["embedded"])
    assert emb.shape == (800, 2) and np.isfinite(emb).all() and data["uwot"]["n_epochs"] == 500
    data = gficf_amd.clustcells(data, from_embedded=True, verbose=False)
    assert len(data["community"]) == 800 and data["community"].min() == 1


@pytest.mark.parametrize("metric", ["manhattan", "cosine", "correlation"])
def test_other_metrics_and_random_init(metric):
    _, _, cells = uc.quality_input()
    data = gficf_amd.runReduction(_pca_data(cells[:, :8]), metric=metric, init="random", n_epochs=30, n_neighbors=10, verbose=False)
    assert np.isfinite(np.asarray(data["embedded"])).all() and data["uwot"]["metric"] == metric


# ------------------------------------------------------------------------------------------------ errors
def test_errors():
    X = uc.random_input()
    Y0 = uc.plane_init(X)
    bad = Y0.copy()
    bad[17, 1] = np.nan
    with pytest.raises(GficfError) as e:
        gficf_amd.umap(X, bad, n_epochs=5)
    assert e.value.status == "GFICF_ERR_BAD_VALUE"
    with pytest.raises(GficfError) as e:
        gficf_amd.runReduction(_pca_data(X), init=bad, n_epochs=5, verbose=False)
    assert e.value.status == "GFICF_ERR_BAD_VALUE"
    P, _ = uc.layout_graph("rand")
    with pytest.raises(GficfError) as e:
        gficf_amd.umap_layout(P, bad, 5)
    assert e.value.status == "GFICF_ERR_BAD_VALUE"
    for k in (129, 258, 1):
        with pytest.raises(GficfError) as e:
            gficf_amd.umap(X, Y0, n_neighbors=k, n_epochs=5)
        assert e.value.status == "GFICF_ERR_INVALID_ARG", k
    with pytest.raises(GficfError) as e:
        gficf_amd.runReduction(_pca_data(X[:100]), n_neighbors=101, verbose=False)
    assert e.value.status == "GFICF_ERR_INVALID_ARG"
    with pytest.raises(GficfError) as e:
        gficf_amd.umap_layout(P, Y0, 5, epoch_begin=3, epoch_end=2)
    assert e.value.status == "GFICF_ERR_INVALID_ARG"
    assert np.isfinite(gficf_amd.umap(X, Y0, n_epochs=5)["embedding"]).all()         # the context is still good
