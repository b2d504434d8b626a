"""SLM on the device (include/gficf_slm.h, libgficf_slm.so): the small ends, the pin to the reference's own algorithm 3
(tests/golden/slm_reference_runs.npz), determinism and structure of the run, the errors, and clustcells(community_algo = "slm")."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gficf_amd
from oracle import oracle_np
from tests.helpers import leiden_cases, leiden_np, slm_cases, slm_par, slm_reference_runs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def check_labels(A, lab, res):
    """Louvain's label conventions and the reported figures."""
    N = A.shape[0]
    assert lab.shape == (N,) and lab.dtype == np.int32 and lab.min() == 0 and lab.max() == lab.n_clusters - 1
    sizes = np.bincount(lab, minlength=lab.n_clusters)
    assert (sizes > 0).all() and (np.diff(sizes) <= 0).all()
    first = np.full(lab.n_clusters, N)
    np.minimum.at(first, np.asarray(lab), np.arange(N))
    assert all(first[c] < first[c + 1] for c in range(lab.n_clusters - 1) if sizes[c] == sizes[c + 1])      # ties by smallest member
    q = oracle_np.modularity_np(A, lab, res)
    print("modularity reported", lab.modularity, "restated", q, "clusters", lab.n_clusters, "start", lab.start, "iterations", lab.iterations)
    assert abs(lab.modularity - q) < 1e-9


def on_device(ops, A, res, n_start, n_iter, seed=0, init=None):
    A = sp.csc_matrix(A)
    N = A.shape[0]
    ptr, idx, x = (torch.from_numpy(a).to(DEV) for a in (A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.astype(np.float64)))
    ws = torch.zeros(ops.slm_workspace_bytes(N, A.nnz), dtype=torch.uint8, device=DEV)
    lab = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    start = None if init is None else torch.from_numpy(np.ascontiguousarray(init, dtype=np.int32)).to(DEV)
    out = ops.slm(N, ptr, idx, x, res, n_start, n_iter, lab, ws, seed, start)
    return lab.cpu().numpy(), out


def test_small_ends():
    one = gficf_amd.slm(sp.csc_matrix((1, 1)), 1.0)
    assert one.tolist() == [0] and one.n_clusters == 1 and one.modularity == 0.0
    loop = gficf_amd.slm(sp.csc_matrix(np.ones((1, 1))), 1.0)                # N = 1 with a stored diagonal: no edge either
    assert loop.tolist() == [0] and loop.n_clusters == 1 and loop.modularity == 0.0
    empty = gficf_amd.slm(sp.csc_matrix((7, 7)), 1.0)
    assert empty.n_clusters == 7 and empty.tolist() == list(range(7)) and empty.modularity == 0.0
    sub = gficf_amd.slm_submove(sp.csc_matrix((7, 7)), np.zeros(7, dtype=np.int32))
    assert sub.tolist() == list(range(7)) and sub.n_clusters == 7
    # two triangles and a bridge
    T = np.zeros((6, 6))
    T[:3, :3] = T[3:, 3:] = 1.0
    T[2, 3] = T[3, 2] = 1.0
    T = sp.csc_matrix(T)                                                     # (the diagonals are stored: they are ignored)
    two = gficf_amd.slm(T, 1.0)
    assert two.tolist() == [0, 0, 0, 1, 1, 1] and abs(two.modularity - oracle_np.modularity_np(T, two, 1.0)) < 1e-12
    assert two.start == 0 and 1 <= two.iterations <= 10      # (the restatement counts fragile ties on unit weights: no trace is compared)
    # a triangle, a pair, and vertices 5 and 6 without an edge
    I = np.zeros((7, 7))
    I[:3, :3] = 1.0
    I[3, 4] = I[4, 3] = 1.0
    I = sp.csc_matrix(I)
    iso = gficf_amd.slm(I, 1.0)
    assert iso.tolist() == [0, 0, 0, 1, 1, 2, 3]
    check_labels(I, iso, 1.0)
    assert gficf_amd.slm_submove(I, np.zeros(7, dtype=np.int32)).tolist()[5:] == [5, 6]      # nothing to move along: they stay alone


def test_hub_graph_through_the_fenced_workgroup_kernel():
    """A 5 000-entry row (five passes of the workgroup form) and a 300-entry one, under a fence that cuts both."""
    A = leiden_cases.hub_graph()
    N = A.shape[0]
    assert np.diff(A.indptr).max() == 5000
    lab = gficf_amd.slm(A, 0.8, 1, 10, 0)
    check_labels(A, lab, 0.8)                                       # (SLM, unlike Leiden, does not promise connected communities)
    P = slm_cases.three_communities(A, A.indptr, A.indices)
    sub = gficf_amd.slm_submove(A, P, 0.8)
    want, n_sub, passes, fragile = slm_par.submove(A, P, 0.8)
    print("hub graph: sub-communities", sub.n_clusters, n_sub, "passes", sub.passes, passes, "fragile", fragile, "differ", int((np.asarray(sub) != want).sum()))
    assert len(set(zip(sub.tolist(), P.tolist()))) == sub.n_clusters        # inside the fence
    assert (np.asarray(sub)[np.asarray(sub)] == np.asarray(sub)).all() and (np.asarray(sub) <= np.arange(N)).all()
    assert fragile == 0 and np.array_equal(sub, want) and sub.n_clusters == n_sub and sub.passes == passes


@pytest.mark.parametrize("key", slm_cases.REFERENCE_CASES)
def test_pinned_to_the_reference(key):
    A, res = slm_cases.reference_input(key)
    ref, printed = slm_reference_runs.slm_reference(key, A, res)
    q_ref = oracle_np.modularity_np(A, ref, res)
    assert abs(printed - q_ref) < 6e-5
    for n_start in (10, 1):
        lab = gficf_amd.slm(A, res, n_start=n_start)
        check_labels(A, lab, res)
        q = oracle_np.modularity_np(A, lab, res)
        print(key, "n_start", n_start, "Q", q, "reference", q_ref, "clusters", lab.n_clusters, int(ref.max()) + 1)
        assert q >= q_ref - slm_cases.Q_TOL, (key, n_start, q, q_ref)


def test_determinism_and_structure():
    ops = gficf_amd.HipOps(0)
    A, res = leiden_cases.exact_inputs()["knn_noise_alg2"]
    N = A.shape[0]
    a, b = gficf_amd.slm(A, res, 3, 4, 5), gficf_amd.slm(A, res, 3, 4, 5)
    assert np.array_equal(a, b) and (a.modularity, a.n_clusters, a.start, a.iterations) == (b.modularity, b.n_clusters, b.start, b.iterations)
    check_labels(A, a, res)
    # HipOps.slm equals slm
    lab, (nc, q, s, it) = on_device(ops, A, res, 3, 4, 5)
    assert np.array_equal(lab, a) and (q, nc, s, it) == (a.modularity, a.n_clusters, a.start, a.iterations)
    # starts together equal starts one by one, ties to the first
    singles = [gficf_amd.slm(A, res, 1, 4, 5 + s) for s in range(3)]
    best = max(range(3), key=lambda s: (singles[s].modularity, -s))
    assert a.start == best and np.array_equal(a, singles[best]) and a.modularity == singles[best].modularity and a.iterations == singles[best].iterations
    # resume equals whole
    one, two = gficf_amd.slm(A, res, 1, 1, 5), gficf_amd.slm(A, res, 1, 2, 5)
    resumed = gficf_amd.slm(A, res, 1, 1, 5, init=one)
    assert np.array_equal(resumed, two) and resumed.modularity == two.modularity
    # init spelled two ways gives one answer
    P = np.asarray(gficf_amd.run_modularity_clustering(A, 1, res, 1, 1, 10, 0)).astype(np.int32)
    x, y = gficf_amd.slm(A, res, 2, 3, 1, init=P), gficf_amd.slm(A, res, 2, 3, 1, init=((N - 1) - P).astype(np.int32))
    assert np.array_equal(x, y) and x.modularity == y.modularity and x.iterations == y.iterations
    # the early stop: the run that stopped is the run that did not
    B, res_b = leiden_cases.exact_inputs()["planted8_res08"]
    full = gficf_amd.slm(B, res_b, 1, 10, 0)
    assert full.iterations == slm_par.slm(B, res_b, 1, 10, 0).iterations < 10
    again = gficf_amd.slm(B, res_b, 1, 1, 0, init=full)
    assert np.array_equal(again, full) and again.modularity == full.modularity


def test_errors_leave_the_next_call_right():
    ops = gficf_amd.HipOps(0)
    A, res = leiden_cases.exact_inputs()["planted3"]
    N = A.shape[0]
    good = gficf_amd.slm(A, res, 1, 2, 0)
    bad = A.copy()
    bad.data[3] = np.nan
    with pytest.raises(gficf_amd.GficfError, match="BAD_VALUE"):
        gficf_amd.slm(bad, res)
    assert np.array_equal(gficf_amd.slm(A, res, 1, 2, 0), good)
    with pytest.raises(gficf_amd.GficfError, match="BAD_VALUE"):
        gficf_amd.slm_submove(bad, np.zeros(N, dtype=np.int32), res)
    bad = A.copy()
    bad.indices[5] = N + 9
    bad.has_sorted_indices = True
    with pytest.raises(gficf_amd.GficfError, match="BAD_CSC"):
        gficf_amd.slm(bad, res)
    assert np.array_equal(gficf_amd.slm(A, res, 1, 2, 0), good)
    with pytest.raises(gficf_amd.GficfError, match="BAD_ID"):
        on_device(ops, A, res, 1, 2, 0, init=np.full(N, N, dtype=np.int32))
    lab, out = on_device(ops, A, res, 1, 2, 0)
    assert np.array_equal(lab, good) and out[1] == good.modularity
    for n_start, n_iter, r in ((0, 2, res), (1, 0, res), (1, 2, -1.0)):
        with pytest.raises(gficf_amd.GficfError, match="INVALID_ARG"):
            on_device(ops, A, r, n_start, n_iter)
    assert np.array_equal(gficf_amd.slm(A, res, 1, 2, 0), good)


def test_clustcells_slm():
    """clustcells(community_algo = "slm"): the blobs come back as the clusters, with what "louvian 2" fills, and the labels are slm()'s."""
    from gficf_amd import synth

    rng = np.random.default_rng(8)
    N, C, d, G = 2000, 10, 12, 300
    truth = rng.integers(0, C, N)
    X = rng.normal(size=(C, d))[truth] * 6.0 + rng.normal(size=(N, d))
    cp, ri, x = synth.counts_csc(G, N, seed=3)
    M = sp.csc_matrix((x, ri, cp), shape=(G, N))
    data = gficf_amd.clustcells({"pca": {"cells": X}, "gficf": M}, k=15, community_algo="slm", verbose=False, n_start=2, seed=7)
    assert leiden_np.same_partition(data["community"], truth) and data["community"].min() == 1
    assert data["cluster.gene.rnk"].shape == (G, C) and sorted(data["cluster.labels"]) == sorted(str(c) for c in range(1, C + 1))
    assert data["cell.adjacency"].shape == (N, N) and len(data["cell.graph"]["weight"]) > 0
    other = gficf_amd.clustcells({"pca": {"cells": X}, "gficf": M}, k=15, community_algo="louvian 2", verbose=False, n_start=2, seed=7)
    assert set(other) == set(data)
    A = gficf_amd.jaccard_adjacency(gficf_amd.clustcells_graph(X, 15, "manhattan"), N)
    lab = gficf_amd.slm(A, 0.8, 2, 10, 7)
    assert np.array_equal(np.asarray(lab) + 1, data["community"]) and lab.modularity == data["modularity"]
    bare = gficf_amd.clustcells({"pca": {"cells": X}}, k=15, community_algo="slm", verbose=False, store_graph=False, n_start=2, seed=7)
    assert np.array_equal(bare["community"], data["community"]) and "cell.graph" not in bare
