"""Leiden on the device (include/gficf_leiden.h, libgficf_leiden.so) — clustcells(community.algo = "leiden"), reference
R/clustCells.R:100-107.

RELAXED CONTRACT, as the header states it: the algorithm and its objective are Leiden's, the visiting order and the random bits are
not leidenalg's.  The objective is Louvain's Q, so the yardsticks of tests/test_louvain_gpu.py apply unchanged: the restated
quality function (oracle_np.modularity_np), the reference optimiser's stored runs (tests/golden/), and Q_TOL = 0.01, which the
reference's own spread across seeds sets there.  New here: every community is connected, the refinement's invariants
(tests/helpers/leiden_np.py: refine_leftover), and resumption (n_iterations = 2 == 1 + 1)."""
import numpy as np
import pytest
import scipy.sparse as sp

import gficf_amd
from oracle import oracle_np
from tests.helpers import closed_form, leiden_cases, leiden_np, reference_runs

pytestmark = pytest.mark.gpu

Q_TOL = 0.01           # tests/test_louvain_gpu.py: the reference's own results span 0.012 across 12 seeds on the worst graph of its sweep
LIVE_CASES = [(6000, 15, 15, 12, 0.8), (8000, 10, 50, 1, 1.0)]
same_partition = leiden_np.same_partition


def check_labels(A, lab, res):
    """Louvain's label conventions, and what Leiden adds: every community is connected."""
    N = A.shape[0]
    assert lab.shape == (N,) and lab.dtype == np.int32 and lab.min() == 0 and lab.max() == lab.n_clusters - 1
    sizes = np.bincount(lab, minlength=lab.n_clusters)
    assert (sizes > 0).all() and (np.diff(sizes) <= 0).all()
    first = np.full(lab.n_clusters, N)
    np.minimum.at(first, np.asarray(lab), np.arange(N))
    assert all(first[c] < first[c + 1] for c in range(lab.n_clusters - 1) if sizes[c] == sizes[c + 1])      # ties by first vertex
    q = oracle_np.modularity_np(A, lab, res)
    print("modularity reported", lab.modularity, "restated", q, "clusters", lab.n_clusters)
    assert abs(lab.modularity - q) < 1e-9
    assert leiden_np.communities_connected(A, lab)


def knn_graph(N, d, k, C, seed, spread=3.0):
    """As tests/test_louvain_gpu.py builds it (the stored reference runs are keyed by the matrix's digest)."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(C, d))[rng.integers(0, C, N)] * spread + rng.normal(size=(N, d))
    edges = gficf_amd.clustcells_graph(X, k, "manhattan")
    return gficf_amd.jaccard_adjacency(edges, N)


@pytest.mark.parametrize("name", ["knn_blobs", "knn_noise_alg2", "planted3", "planted8_res08"])
def test_golden_graphs(name):
    A, res, ref = leiden_cases.golden()[name]
    lab = gficf_amd.leiden(A, res, 2)
    check_labels(A, lab, res)
    q_ref = oracle_np.modularity_np(A, ref, res)
    print(name, "Q", lab.modularity, "reference", q_ref)
    assert lab.modularity >= q_ref - Q_TOL, (name, lab.modularity, q_ref)
    if name != "knn_noise_alg2":
        assert same_partition(lab, ref), name


@pytest.mark.parametrize("c,m", leiden_cases.RINGS)
def test_rings(c, m):
    A, clique = leiden_cases.ring(c, m)
    lab = gficf_amd.leiden(A, 0.8, 2)
    check_labels(A, lab, 0.8)
    assert lab.n_clusters == c and same_partition(lab, clique)
    assert abs(lab.modularity - leiden_np.modularity(A, clique, 0.8)) < 1e-9
    assert abs(lab.modularity - closed_form.ring_of_cliques_modularity(c, m, 0.8)) < 1e-9


@pytest.mark.parametrize("c,m", leiden_cases.RINGS)
def test_a_disconnected_start_is_split(c, m):
    A, clique, init = leiden_cases.disconnected_start(c, m)
    assert same_partition(leiden_np.local_moving(A, init, 0.8), init)          # local moving alone keeps the two-component community
    R = gficf_amd.leiden_refine(A, init, 0.8)
    assert R.dtype == np.int32 and len(np.unique(R)) == c and same_partition(R, clique)
    assert leiden_np.communities_connected(A, R) and len(np.unique(np.stack([R, init], axis=1), axis=0)) == c
    lab = gficf_amd.leiden(A, 0.8, 1, init=init)
    check_labels(A, lab, 0.8)
    print("Q", lab.modularity, "Q(init)", leiden_np.modularity(A, init, 0.8))
    assert lab.modularity >= leiden_np.modularity(A, init, 0.8)


@pytest.mark.parametrize("name", ["knn_noise_alg2", "knn_blobs"])
@pytest.mark.parametrize("start", ["louvain", "one community"])
def test_refinement_invariants(name, start):
    A, res, _ = leiden_cases.golden()[name]
    N = A.shape[0]
    P = np.asarray(gficf_amd.run_modularity_clustering(A, 1, res, 1, 1, 10, 0)) if start == "louvain" else np.zeros(N, dtype=np.int32)
    R = gficf_amd.leiden_refine(A, P, res)
    assert R.shape == (N,) and R.dtype == np.int32
    assert len(np.unique(np.stack([R, P], axis=1), axis=0)) == len(np.unique(R))        # every refined community inside one community of P
    assert leiden_np.communities_connected(A, R)
    left = leiden_np.refine_leftover(A, P, R, res, 1e-6)
    print(name, start, "refined communities", len(np.unique(R)), "of", N, "leftover", left)
    assert left == 0
    assert len(np.unique(R)) < N
    assert np.array_equal(R, leiden_np.canonical(R))                                    # the label is the smallest member
    assert np.array_equal(R, gficf_amd.leiden_refine(A, P, res))


def test_long_rows():
    """Hubs of 5 000 and 300 neighbours, each neighbour its own community at the start: the workgroup path, several passes over a row."""
    A = leiden_cases.hub_graph()
    lab = gficf_amd.leiden(A, 1.0, 2)
    check_labels(A, lab, 1.0)
    q_np = leiden_np.modularity(A, leiden_np.leiden(A, 1.0, 2), 1.0)
    print("Q", lab.modularity, "restatement", q_np)
    assert lab.modularity >= q_np - Q_TOL


def test_determinism_and_resumption():
    A, res, ref = leiden_cases.golden()["knn_noise_alg2"]
    two = gficf_amd.leiden(A, res, 2)
    again = gficf_amd.leiden(A, res, 2)
    assert np.array_equal(two, again) and two.modularity == again.modularity and two.n_clusters == again.n_clusters
    one = gficf_amd.leiden(A, res, 1)
    resumed = gficf_amd.leiden(A, res, 1, init=one)
    assert np.array_equal(two, resumed) and two.modularity == resumed.modularity
    other = gficf_amd.leiden(A, res, 2, seed=1234)
    check_labels(A, other, res)
    q_ref = oracle_np.modularity_np(A, ref, res)
    print("Q seed 0", two.modularity, "seed 1234", other.modularity, "reference", q_ref)
    assert other.modularity >= q_ref - Q_TOL


@pytest.mark.parametrize("N,d,k,C,res", LIVE_CASES)
def test_live_knn_graphs_against_stored_reference_runs(N, d, k, C, res):
    """kNN -> Jaccard -> adjacency on the device, then Leiden; k = 50 gives vertices of degree > 128 (workgroup path)."""
    A = knn_graph(N, d, k, C, seed=N + k)
    lab = gficf_amd.leiden(A, res, 2)
    check_labels(A, lab, res)
    ref_labels, printed = reference_runs.modularity_reference(f"live_N{N}_d{d}_k{k}_C{C}_res{res}", A, res, 1, 1, 10, 0)
    q_ref = oracle_np.modularity_np(A, ref_labels, res)
    print("Q", lab.modularity, "reference", q_ref, "largest row", int(np.diff(A.indptr).max()))
    assert abs(q_ref - printed) < 6e-5
    assert lab.modularity >= q_ref - Q_TOL, (lab.modularity, q_ref)


def test_edge_cases():
    one = gficf_amd.leiden(sp.csc_matrix((1, 1)), 1.0)
    assert one.tolist() == [0] and one.n_clusters == 1
    empty = gficf_amd.leiden(sp.csc_matrix((7, 7)), 1.0)
    want = gficf_amd.run_modularity_clustering(sp.csc_matrix((7, 7)), 1, 1.0, 1, 1, 1, 0, False)
    assert empty.n_clusters == 7 and sorted(empty.tolist()) == list(range(7)) and empty.modularity == want.modularity
    tri = np.zeros((7, 7))
    tri[:3, :3] = 1.0
    tri[3, 4] = tri[4, 3] = 1.0                                   # a triangle, a pair, and vertices 5 and 6 without an edge
    tri = sp.csc_matrix(tri)                                      # (the triangle's diagonal is stored: it is ignored)
    two = gficf_amd.leiden(tri, 1.0)
    assert two.tolist() == [0, 0, 0, 1, 1, 2, 3] and abs(two.modularity - oracle_np.modularity_np(tri, two, 1.0)) < 1e-12
    A, res, _ = leiden_cases.golden()["planted3"]
    B = (A + sp.identity(A.shape[0], format="csc") * 0.5).tocsc()
    B.sort_indices()
    plain, with_diag = gficf_amd.leiden(A, res), gficf_amd.leiden(B, res)
    assert np.array_equal(plain, with_diag) and plain.modularity == with_diag.modularity
    # the device entries on resident tensors give the host entries' answer
    import torch

    ops = gficf_amd.HipOps(0)
    dev = "cuda:0"
    ptr = torch.from_numpy(A.indptr.astype(np.int64)).to(dev)
    idx = torch.from_numpy(A.indices.astype(np.int32)).to(dev)
    x = torch.from_numpy(A.data.astype(np.float64)).to(dev)
    ws = torch.zeros(ops.leiden_workspace_bytes(A.shape[0], A.nnz), dtype=torch.uint8, device=dev)
    lab = torch.zeros(A.shape[0], dtype=torch.int32, device=dev)
    nc, q = ops.leiden(A.shape[0], ptr, idx, x, res, 2, lab, ws)
    assert nc == plain.n_clusters and q == plain.modularity and np.array_equal(lab.cpu().numpy(), plain)
    refined = torch.zeros(A.shape[0], dtype=torch.int32, device=dev)
    nr = ops.leiden_refine(A.shape[0], ptr, idx, x, res, lab, refined, ws)
    R = gficf_amd.leiden_refine(A, plain, res)
    assert np.array_equal(refined.cpu().numpy(), R) and nr == len(np.unique(R))
    # bad input is reported, not followed
    bad = A.copy()
    bad.data[3] = np.nan
    with pytest.raises(gficf_amd.GficfError):
        gficf_amd.leiden(bad, res)
    bad = A.copy()
    bad.indices[5] = A.shape[0] + 9
    bad.has_sorted_indices = True
    with pytest.raises(gficf_amd.GficfError):
        gficf_amd.leiden(bad, res)
    with pytest.raises(gficf_amd.GficfError):
        ops.leiden(A.shape[0], ptr, idx, x, res, 0, lab, ws)
    with pytest.raises(gficf_amd.GficfError):
        ops.leiden(A.shape[0], ptr, idx, x, -1.0, 2, lab, ws)
    with pytest.raises(gficf_amd.GficfError):
        ops.leiden(A.shape[0], ptr, idx, x, res, 2, lab, ws, init=torch.full((A.shape[0],), A.shape[0], dtype=torch.int32, device=dev))


def test_clustcells_leiden():
    """clustcells(community_algo = "leiden"): planted cell types come back as the clusters; without the stored graph the same labels."""
    from gficf_amd import synth

    rng = np.random.default_rng(8)
    N, C, d, G = 3000, 5, 12, 400
    truth = rng.integers(0, C, N)
    X = rng.normal(size=(C, d))[truth] * 6.0 + rng.normal(size=(N, d))
    cp, ri, x = synth.counts_csc(G, N, seed=3)
    M = sp.csc_matrix((x, ri, cp), shape=(G, N))
    data = gficf_amd.clustcells({"pca": {"cells": X}, "gficf": M}, k=15, community_algo="leiden", verbose=False)
    assert same_partition(data["community"], truth) and data["community"].min() == 1
    assert data["cluster.gene.rnk"].shape == (G, C) and sorted(data["cluster.labels"]) == sorted(str(c) for c in range(1, C + 1))
    assert data["cell.adjacency"].shape == (N, N) and len(data["cell.graph"]["weight"]) > 0
    bare = gficf_amd.clustcells({"pca": {"cells": X}}, k=15, community_algo="leiden", verbose=False, store_graph=False)
    assert np.array_equal(bare["community"], data["community"]) and bare["modularity"] == data["modularity"]
    assert "cell.graph" not in bare and "cell.adjacency" not in bare
    with pytest.raises(ValueError):
        gficf_amd.clustcells({"pca": {"cells": X}}, community_algo="walktrap")
