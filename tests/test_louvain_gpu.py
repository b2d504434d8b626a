"""Scope row N4: community detection on the Jaccard graph — RunModularityClustering(adjacency, 1, resolution, 1, ...)
(reference R/clustCells.R:80,86 -> src/RModularityOptimizer.cpp:25 -> src/ModularityOptimizer.cpp:594-612).

RELAXED CONTRACT, stated here as include/gficf_hip.h states it: the reference is sequential and seed-exact, the device
form is a deterministic parallel Louvain on the SAME objective.  What is tested:
  * against the reference's own outputs (tests/golden/louvain_cases.npz, made by running a build of the reference's
    src/ModularityOptimizer.cpp; on the graphs built here, tests/golden/louvain_reference_runs.npz, and the same binary live,
    oracle/_ref/, when it is there: tests/helpers/reference_runs.py): modularity not more than
    Q_TOL below the reference's, the same partition where the structure is unambiguous (planted partitions);
  * the modularity the call reports == the restated quality function (oracle_np.modularity_np, itself pinned to the
    reference's print-out) of the labels it returns, to 1e-9;
  * label conventions (0-based, clusters by decreasing size), bit-reproducibility, the resolution parameter, edge cases."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse import csgraph

import gficf_amd
from oracle import oracle_np
from tests.helpers import reference_runs

pytestmark = pytest.mark.gpu

Q_TOL = 0.01           # device modularity >= reference modularity - Q_TOL.  Measured over a sweep of 72 kNN -> Jaccard graphs
                       # (tools/louvain_sweep.py): device - reference(seed 0) in [-0.0065, +0.0345], mean +0.0004; the reference's
                       # own results on the worst of them span 0.012 across 12 seeds, which is what sets the tolerance


def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "louvain_cases.npz"))
    names = sorted({k.split("/")[0] for k in z.files})
    for n in names:
        N = len(z[n + "/indptr"]) - 1
        A = sp.csc_matrix((z[n + "/data"], z[n + "/indices"], z[n + "/indptr"]), shape=(N, N))
        yield n, A, z[n + "/params"], z[n + "/labels"], float(z[n + "/printed_q"][0])


def same_partition(a, b):
    pairs = np.unique(np.stack([a, b], axis=1), axis=0)
    return len(pairs) == len(np.unique(a)) == len(np.unique(b))


def check_labels(A, lab, res):
    N = A.shape[0]
    assert lab.shape == (N,) and lab.dtype == np.int32 and lab.min() == 0 and lab.max() == lab.n_clusters - 1
    sizes = np.bincount(lab, minlength=lab.n_clusters)
    assert (sizes > 0).all() and (np.diff(sizes) <= 0).all()                 # orderClustersByNNodes
    assert abs(lab.modularity - oracle_np.modularity_np(A, lab, res)) < 1e-9
    # exact, whatever the optimum: a vertex only ever joins a community it has an edge to, or leaves for its own id, so no cluster spans two
    # connected components of the graph (off-diagonal, positive entries), and a vertex without an edge is alone in its cluster
    C = sp.coo_matrix(A)
    edge = (C.row != C.col) & (C.data > 0)
    G = sp.csr_matrix((np.ones(int(edge.sum()), dtype=np.int8), (C.row[edge], C.col[edge])), shape=(N, N))
    n_comp, comp = csgraph.connected_components(G, directed=False)
    assert len(np.unique(np.asarray(lab, dtype=np.int64) * n_comp + comp)) == lab.n_clusters
    alone = (np.bincount(C.row[edge], minlength=N) + np.bincount(C.col[edge], minlength=N)) == 0
    assert (sizes[np.asarray(lab)[alone]] == 1).all()


def test_against_reference_outputs(golden_dir):
    seen = 0
    for name, A, (res, alg, n_start, n_iter, seed), ref_labels, printed in golden(golden_dir):
        q_ref = oracle_np.modularity_np(A, ref_labels, res)
        assert abs(q_ref - printed) < 6e-5                                    # the restatement vs the reference's print-out
        lab = gficf_amd.run_modularity_clustering(A, 1, res, int(alg), int(n_start), int(n_iter), int(seed), False)
        check_labels(A, lab, res)
        assert lab.modularity >= q_ref - Q_TOL, (name, lab.modularity, q_ref)
        if name.startswith("planted") or name == "knn_blobs":
            assert same_partition(lab, ref_labels), name                     # unambiguous structure: the same clusters
            assert np.array_equal(np.bincount(lab), np.bincount(ref_labels))
        seen += 1
    assert seen == 4


def knn_graph(N, d, k, C, seed, spread=3.0):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(C, d))[rng.integers(0, C, N)] * spread + rng.normal(size=(N, d))
    edges = gficf_amd.clustcells_graph(X, k, "manhattan")
    return gficf_amd.jaccard_adjacency(edges, N)


def hub_graph():
    """Hubs with 3 000 and 30 000 neighbours, every leaf also on a ring (test_hub_vertices_beyond_the_table)."""
    rng = np.random.default_rng(21)
    N = 40000
    rows, cols, vals = [], [], []
    for hub, deg in ((0, 30000), (1, 3000)):
        leaves = rng.choice(np.arange(2, N), deg, replace=False)
        rows += [np.full(deg, hub)]; cols += [leaves]; vals += [rng.integers(1, 32, deg) / 64.0]
    ring = np.arange(2, N)                                           # every leaf also sits on a ring: no isolated vertices
    rows += [ring]; cols += [np.roll(ring, -1)]; vals += [np.full(N - 2, 0.5)]
    W = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N)).tocsc()
    A = (W + W.T).tocsc()
    A.sum_duplicates(); A.sort_indices()
    return A


LIVE_CASES = [(6000, 15, 15, 12, 0.8), (20000, 20, 30, 1, 0.8), (8000, 10, 50, 1, 1.0), (12000, 8, 10, 3, 2.0)]
FUNCTION2_CASES = [(6000, 15, 10, 0.05), (8000, 20, 1, 0.02)]


@pytest.mark.parametrize("N,d,k,C,res", LIVE_CASES)
def test_live_against_the_reference_binary(N, d, k, C, res):
    """The full chain on the device (kNN -> Jaccard -> filter -> adjacency -> Louvain) against the reference's optimiser run
    on the same adjacency matrix.  k = 50 and the structureless cases give vertices of degree > 128 (workgroup path)."""
    A = knn_graph(N, d, k, C, seed=N + k)
    lab = gficf_amd.run_modularity_clustering(A, 1, res, 1, 1, 10, 0, False)
    check_labels(A, lab, res)
    ref_labels, printed = reference_runs.modularity_reference(f"live_N{N}_d{d}_k{k}_C{C}_res{res}", A, res, 1, 1, 10, 0)
    q_ref = oracle_np.modularity_np(A, ref_labels, res)
    assert abs(q_ref - printed) < 6e-5
    assert lab.modularity >= q_ref - Q_TOL, (lab.modularity, q_ref)
    assert 0.5 * (ref_labels.max() + 1) <= lab.n_clusters <= 2 * (ref_labels.max() + 1)
    again = gficf_amd.run_modularity_clustering(A, 1, res, 1, 1, 10, 0, False)
    assert np.array_equal(lab, again) and lab.modularity == again.modularity    # bit-reproducible


def test_large_graph_200k_cells_against_the_reference():
    """200 k cells, k = 30 (9 M adjacency entries): label conventions, reported Q, reproducibility, and the reference's
    modularity on the same matrix (its binary takes a few seconds on one core)."""
    A = knn_graph(200000, 20, 30, 40, seed=77, spread=2.0)
    lab = gficf_amd.run_modularity_clustering(A, 1, 0.8, 1, 1, 10, 0, False)
    check_labels(A, lab, 0.8)
    again = gficf_amd.run_modularity_clustering(A, 1, 0.8, 1, 1, 10, 0, False)
    assert np.array_equal(lab, again)
    ref_labels, printed = reference_runs.modularity_reference("large_200k", A, 0.8, 1, 1, 10, 0)
    q_ref = oracle_np.modularity_np(A, ref_labels, 0.8)
    assert abs(q_ref - printed) < 6e-5 and lab.modularity >= q_ref - Q_TOL, (lab.modularity, q_ref)


@pytest.mark.parametrize("N,k,C,res", FUNCTION2_CASES)
def test_alternative_modularity_function(N, k, C, res):
    """RunModularityClustering(modularity = 2): unit node weights, the resolution taken as it is (reference
    src/RModularityOptimizer.cpp:36,100; never chosen by clustcells()).  Against the reference binary run with the same function."""
    A = knn_graph(N, 10, k, C, seed=N + k)
    lab = gficf_amd.run_modularity_clustering(A, 2, res, 1, 1, 10, 0, False)
    assert abs(lab.modularity - oracle_np.modularity_np(A, lab, res, 2)) < 1e-9
    sizes = np.bincount(lab)
    assert lab.min() == 0 and (sizes > 0).all() and (np.diff(sizes) <= 0).all()
    std = gficf_amd.run_modularity_clustering(A, 1, 0.8, 1, 1, 10, 0, False)            # the context is back on the standard function
    assert abs(std.modularity - oracle_np.modularity_np(A, std, 0.8)) < 1e-9
    ref_labels, printed = reference_runs.modularity_reference(f"function2_N{N}_k{k}_C{C}_res{res}", A, res, 1, 1, 10, 0, function=2)
    q_ref = oracle_np.modularity_np(A, ref_labels, res, 2)
    assert abs(q_ref - printed) < 6e-5                                                  # the restatement vs the reference's print-out
    assert lab.modularity >= q_ref - Q_TOL, (lab.modularity, q_ref)
    with pytest.raises(ValueError):
        gficf_amd.run_modularity_clustering(A, 2, 1.5)


@pytest.mark.parametrize("c,m,weight,n_start", [(60, 10, 1.0, 1), (60, 10, 0.37, 10), (1000, 40, 1.0, 1), (1000, 40, 2.5, 10), (8, 5, 1.0, 10),
                                                 (1, 6, 1.0, 3)])
def test_ring_of_cliques_against_the_derived_partition_and_modularity(c, m, weight, n_start):
    """An answer by counting, no oracle and no reference binary in the loop (tests/helpers/closed_form.py): c cliques of m vertices on a ring, one
    edge between neighbours.  For c < resolution x (m (m - 1) + 2) the optimum is one community per clique and Q = m (m - 1) / (m (m - 1) + 2) -
    resolution / c — the labels must be that partition exactly (whatever the batch of starts), the reported modularity that number."""
    from tests.helpers import closed_form

    res = 0.8
    assert c < res * (m * (m - 1) + 2)
    A, clique = closed_form.ring_of_cliques(c, m, weight)
    lab = gficf_amd.run_modularity_clustering(A, 1, res, 1, n_start, 10, 7)
    check_labels(A, lab, res)
    assert lab.n_clusters == c and same_partition(np.asarray(lab), clique)
    assert abs(lab.modularity - closed_form.ring_of_cliques_modularity(c, m, res)) < 1e-9


def test_hub_vertices_beyond_the_table():
    """Hubs with 3 000 and 30 000 neighbours, each neighbour its own community at the start: more than the 2048- and the
    8192-slot table hold — the second takes several passes over its edges.  Checked against the reference binary."""
    A = hub_graph()
    lab = gficf_amd.run_modularity_clustering(A, 1, 1.0, 1, 1, 10, 0, False)
    check_labels(A, lab, 1.0)
    again = gficf_amd.run_modularity_clustering(A, 1, 1.0, 1, 1, 10, 0, False)
    assert np.array_equal(lab, again)
    ref_labels, _ = reference_runs.modularity_reference("hubs", A, 1.0, 1, 1, 10, 0)
    assert lab.modularity >= oracle_np.modularity_np(A, ref_labels, 1.0) - Q_TOL


def test_resolution_and_iterations():
    A = knn_graph(5000, 10, 15, 1, seed=11)
    coarse = gficf_amd.run_modularity_clustering(A, 1, 0.3, 1, 1, 10, 0, False)
    fine = gficf_amd.run_modularity_clustering(A, 1, 3.0, 1, 1, 10, 0, False)
    assert coarse.n_clusters < fine.n_clusters
    one = gficf_amd.run_modularity_clustering(A, 1, 1.0, 1, 1, 1, 0, False)
    ten = gficf_amd.run_modularity_clustering(A, 1, 1.0, 1, 1, 10, 0, False)
    assert ten.modularity >= one.modularity - 1e-12                            # further passes never lose quality
    # random starts: the best of several is never worse than the first, equal arguments give equal results, the seed matters
    s1 = gficf_amd.run_modularity_clustering(A, 1, 1.0, 1, 1, 10, 0, False)
    s5 = gficf_amd.run_modularity_clustering(A, 1, 1.0, 1, 5, 10, 0, False)
    s5b = gficf_amd.run_modularity_clustering(A, 1, 1.0, 1, 5, 10, 0, False)
    other = gficf_amd.run_modularity_clustering(A, 1, 1.0, 1, 1, 10, 1234, False)
    assert np.array_equal(s1, ten) and s5.modularity >= s1.modularity and np.array_equal(s5, s5b)
    assert not np.array_equal(other, s1)                                       # structureless data: another split, another optimum
    for lab in (s5, other):
        check_labels(A, lab, 1.0)
    # algorithm 2 = the same descent plus one more local moving per level on the way back up: never worse in one pass
    refined = gficf_amd.run_modularity_clustering(A, 1, 1.0, 2, 1, 1, 0, False)
    assert refined.modularity >= one.modularity - 1e-12
    for lab, res in ((coarse, 0.3), (fine, 3.0), (one, 1.0), (ten, 1.0), (refined, 1.0)):
        check_labels(A, lab, res)
    ref_labels, _ = reference_runs.modularity_reference("resolution_alg2", A, 1.0, 2, 1, 10, 0)      # against the reference's algorithm 2
    ref10 = gficf_amd.run_modularity_clustering(A, 1, 1.0, 2, 1, 10, 0, False)
    check_labels(A, ref10, 1.0)
    assert ref10.modularity >= oracle_np.modularity_np(A, ref_labels, 1.0) - Q_TOL


@pytest.mark.parametrize("N,k,C,res,alg,n_start", [(5000, 15, 1, 1.0, 1, 7), (9000, 30, 8, 0.8, 1, 10), (3000, 10, 1, 1.5, 2, 5), (7000, 50, 1, 1.0, 1, 20),
                                                      (60000, 15, 5, 0.8, 1, 3)])
def test_starts_run_together_equal_starts_run_one_by_one(N, k, C, res, alg, n_start, monkeypatch):
    """Round 6: the n.start starts (reference src/RModularityOptimizer.cpp:108-142) run TOGETHER, as one problem on the disjoint union of
    the copies (one launch set; at most 16 at a time, so n_start = 20 is two batches) — a start's descent, its convergence decisions and
    its passes must be exactly those of running it alone: labels, number of clusters and modularity are identical to the run with
    GFICF_LOUVAIN_BATCH=1 (the starts one after the other through the same kernels), and to a batch size that does not divide n_start."""
    A = knn_graph(N, 10, k, C, seed=3 * N + k)
    together = gficf_amd.run_modularity_clustering(A, 1, res, alg, n_start, 10, 4242, False)
    check_labels(A, together, res)
    monkeypatch.setenv("GFICF_LOUVAIN_BATCH", "1")
    one_by_one = gficf_amd.run_modularity_clustering(A, 1, res, alg, n_start, 10, 4242, False)
    monkeypatch.setenv("GFICF_LOUVAIN_BATCH", "3")
    by_three = gficf_amd.run_modularity_clustering(A, 1, res, alg, n_start, 10, 4242, False)
    monkeypatch.delenv("GFICF_LOUVAIN_BATCH")
    for other in (one_by_one, by_three):
        assert np.array_equal(together, other) and together.modularity == other.modularity and together.n_clusters == other.n_clusters
    # the best of the starts is at least as good as each of them alone (start s alone = n_start 1 with that start's seed is not reachable from
    # the API; the first start is: seed and start number 0)
    first = gficf_amd.run_modularity_clustering(A, 1, res, alg, 1, 10, 4242, False)
    assert together.modularity >= first.modularity


def test_device_resident_chain_and_edge_cases():
    import torch

    ops = gficf_amd.HipOps(0)
    A = knn_graph(4000, 10, 15, 6, seed=5)
    dev = "cuda:0"
    ptr = torch.from_numpy(A.indptr.astype(np.int64)).to(dev)
    idx = torch.from_numpy(A.indices.astype(np.int32)).to(dev)
    x = torch.from_numpy(A.data).to(dev)
    ws = torch.zeros(ops.louvain_workspace_bytes(A.shape[0], A.nnz), dtype=torch.uint8, device=dev)
    lab = torch.zeros(A.shape[0], dtype=torch.int32, device=dev)
    nc, q = ops.louvain(A.shape[0], ptr, idx, x, 0.8, 10, lab, ws)
    host = gficf_amd.run_modularity_clustering(A, 1, 0.8, 1, 1, 10, 0, False)
    assert nc == host.n_clusters and q == host.modularity and np.array_equal(lab.cpu().numpy(), host)
    # the diagonal is ignored (src/RModularityOptimizer.cpp:73-75)
    B = (A + sp.identity(A.shape[0], format="csc") * 0.5).tocsc()
    B.sort_indices()
    with_diag = gficf_amd.run_modularity_clustering(B, 1, 0.8, 1, 1, 10, 0, False)
    assert np.array_equal(with_diag, host)
    # no edges: every vertex alone; two components: two clusters
    empty = gficf_amd.run_modularity_clustering(sp.csc_matrix((7, 7)), 1, 1.0, 1, 1, 1, 0, False)
    assert empty.n_clusters == 7 and sorted(empty.tolist()) == list(range(7)) and empty.modularity == 0.0
    tri = sp.csc_matrix(np.array([[0, 1, 1, 0, 0], [1, 0, 1, 0, 0], [1, 1, 0, 0, 0], [0, 0, 0, 0, 1], [0, 0, 0, 1, 0]], dtype=float))
    two = gficf_amd.run_modularity_clustering(tri, 1, 1.0, 1, 1, 10, 0, False)
    assert two.tolist() == [0, 0, 0, 1, 1] and abs(two.modularity - oracle_np.modularity_np(tri, two, 1.0)) < 1e-12
    # bad input is reported, not followed
    bad = A.copy()
    bad.data[3] = np.nan
    with pytest.raises(gficf_amd.GficfError):
        gficf_amd.run_modularity_clustering(bad, 1, 0.8, 1, 1, 1, 0, False)
    bad = A.copy()
    bad.indices[5] = A.shape[0] + 9
    bad.has_sorted_indices = True
    with pytest.raises(gficf_amd.GficfError):
        gficf_amd.run_modularity_clustering(bad, 1, 0.8, 1, 1, 1, 0, False)
    with pytest.raises(ValueError):
        gficf_amd.run_modularity_clustering(A, 3, 0.8)
    with pytest.raises(ValueError):
        gficf_amd.run_modularity_clustering(A, 1, 0.8, 3)


def test_clustcells_end_to_end():
    """clustcells() (R/clustCells.R:46-126) in one call: planted cell types come back as the clusters, the signatures are the
    per-cluster gene sums of the GF-ICF matrix."""
    from gficf_amd import synth

    rng = np.random.default_rng(8)
    N, C, d, G = 3000, 5, 12, 400
    truth = rng.integers(0, C, N)
    X = rng.normal(size=(C, d))[truth] * 6.0 + rng.normal(size=(N, d))
    cp, ri, x = synth.counts_csc(G, N, seed=3)
    M = sp.csc_matrix((x, ri, cp), shape=(G, N))
    for algo in ("louvian", "louvian 2", "louvian 3"):
        data = gficf_amd.clustcells({"pca": {"cells": X}, "gficf": M}, k=15, community_algo=algo, verbose=False)
        assert same_partition(data["community"], truth) and data["community"].min() == 1
        sig, labels = data["cluster.gene.rnk"], data["cluster.labels"]
        assert sig.shape == (G, C) and sorted(labels) == sorted(str(c) for c in range(1, C + 1))
        j = list(labels).index(data["cluster"][0])
        want = np.asarray(M[:, data["cluster"] == data["cluster"][0]].sum(axis=1)).ravel()
        assert np.allclose(sig[:, j], want, rtol=1e-9, atol=1e-9)
        assert data["cell.adjacency"].shape == (N, N) and len(data["cell.graph"]["weight"]) > 0
    # the fused entry (nothing crosses PCIe between the steps) gives the labels of the staged path
    staged = gficf_amd.clustcells({"pca": {"cells": X}}, k=15, community_algo="louvian 2", verbose=False, n_start=2)
    fused = gficf_amd.clustcells({"pca": {"cells": X}}, k=15, community_algo="louvian 2", verbose=False, n_start=2, store_graph=False)
    assert np.array_equal(staged["community"], fused["community"]) and staged["modularity"] == fused["modularity"]
    assert "cell.graph" not in fused
    rngu = np.random.default_rng(4)
    U = rngu.normal(size=(5000, 6))                                       # no structure: many near-ties on the way
    lab = gficf_amd.phenograph(U, 20, "euclidean", 0.8, 1, 1, 10, 0)
    A = gficf_amd.jaccard_adjacency(gficf_amd.clustcells_graph(U, 20, "euclidean"), 5000)
    want = gficf_amd.run_modularity_clustering(A, 1, 0.8, 1, 1, 10, 0, False)
    assert np.array_equal(lab, want) and lab.modularity == want.modularity
    assert lab.n_edges == len(gficf_amd.clustcells_graph(U, 20, "euclidean")["weight"])
    with pytest.raises(ValueError):
        gficf_amd.clustcells({"pca": {"cells": X}}, community_algo="walktrap")
    with pytest.raises(ValueError):
        gficf_amd.clustcells({"gficf": M})
