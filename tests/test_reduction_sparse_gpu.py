"""runReductionSparse on the device: the data$pca-less branch of runReduction equals its stages composed by hand, bit for bit, and
keeps three planted groups of cells apart in the plane.

Data: 600 cells in three groups of 200 over 900 genes; a cell draws 60 of its group's own 300 genes with gamma values and 5 genes
from anywhere, and the matrix goes through gficf().  Statistic: the share of every cell's 10 nearest neighbours in the plane that
belong to its group; the thresholds are those of the embedding tests on data["pca"]: 0.99 (tests/test_umap_gpu.py,
test_quality_of_full_runs) and for t-SNE the port's minimum less its spread over the seeds, 1.0 - 0 (tests/test_tsne_gpu.py,
MEASURED_QUALITY)."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import gficf_amd

pytestmark = pytest.mark.gpu

PURITY = {"tumap": 0.99, "umap": 0.99, "tsne": 1.0}
KW = {"tumap": {"n_epochs": 100}, "umap": {"n_epochs": 100}, "tsne": {"perplexity": 10, "max_iter": 150}}
SEED = 11


def _groups(n_groups=3, per=200, own=300, drawn=60, stray=5, seed=1):
    rng = np.random.default_rng(seed)
    G, N = n_groups * own, n_groups * per
    rows, cols = [], []
    for c in range(N):
        g = c // per
        r = g * own + rng.choice(own, drawn, replace=False)
        if stray:
            r = np.union1d(r, rng.choice(G, stray, replace=False))
        rows.append(r)
        cols.append(np.full(len(r), c))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    return sp.csc_matrix((rng.gamma(2, 1, len(rows)), (rows, cols)), shape=(G, N)), np.repeat(np.arange(n_groups), per)


@pytest.fixture(scope="module")
def planted():
    counts, labels = _groups()
    data = gficf_amd.gficf(counts, normalize=False, verbose=False)
    assert data["gficf"].shape[1] == 600
    return data, labels


def _own_share(Y, labels, k=10):
    """The purity of tests/helpers/umap_np.py, quality(), with 10 neighbours."""
    Y = np.asarray(Y, dtype=np.float64)
    D = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(D, np.inf)
    nn = np.argsort(D, axis=1, kind="stable")[:, :k]
    return float((labels[nn] == labels[:, None]).mean())


def _by_hand_umap(M, reduction, seed, n_epochs, k=15):
    """The stages one after the other, and the components of the graph: the default start is spectral_init on a connected graph
    and the scaled first two components of rsvd on any other."""
    N = M.shape[1]
    nn = gficf_amd.find_nn_sparse(M, k, True, "euclidean")
    P = gficf_amd.fuzzy_simplicial_set(nn["idx"], nn["dist"], 1.0, 1.0)[0]
    n_comp = gficf_amd.graph_components(P)[1]
    if n_comp == 1:
        Y0 = gficf_amd.spectral_init(P, seed=seed)
    else:
        Y0 = gficf_amd.umap_init("pca", gficf_amd.rsvd(M, k=2, centre=True)["cells"], N, seed)
    a, b = (1.0, 1.0) if reduction == "tumap" else gficf_amd.find_ab_params(1.0, 0.01)
    return nn, P, gficf_amd.umap_layout(P, Y0, n_epochs, a, b, 1.0, 5, 1.0, seed=seed), n_comp


@pytest.mark.parametrize("reduction", ("tumap", "umap"))
def test_umap_forms_equal_their_stages_and_keep_the_groups(planted, reduction):
    """The three groups share 5 stray genes in 65 per cell: their 15-neighbour graph falls into three components, so the default
    start is the warned fall-back to "pca" (test_spectral_starts_on_a_connected_graph runs the spectral one)."""
    data, labels = planted
    nn, P, Y, n_comp = _by_hand_umap(data["gficf"], reduction, SEED, 100)
    assert n_comp == 3
    with pytest.warns(UserWarning, match=r"more than one component \(3\)"):
        out = gficf_amd.runReductionSparse({"gficf": data["gficf"]}, reduction=reduction, seed=SEED, verbose=False, **KW[reduction])
    emb = np.asarray(out["embedded"])
    assert list(out["embedded"].columns) == ["X", "Y"] and out["reduction"] == reduction
    assert np.array_equal(emb, Y.astype(np.float64))
    model = out["uwot"]
    assert model["space"] == "gficf" and model["n_neighbors"] == 15 and model["n_epochs"] == 100 and model["seed"] == SEED
    assert np.array_equal(model["nn"]["idx"], nn["idx"]) and np.array_equal(model["nn"]["dist"], nn["dist"])
    assert (model["graph"] != P).nnz == 0 and np.array_equal(model["embedding"], emb)
    if reduction == "tumap":
        assert model["a"] == 1.0 and model["b"] == 1.0
    share = _own_share(emb, labels)
    print(f"{reduction}: own-group share of the 10 nearest neighbours in the plane {share:.4f}")
    assert share >= PURITY[reduction]
    out = gficf_amd.clustcells(out, from_embedded=True, verbose=False)
    assert len(out["community"]) == 600 and out["community"].min() == 1
    with pytest.raises(NotImplementedError, match="runReductionSparse"):
        gficf_amd.embedNewCells(out, sp.csc_matrix((data["gficf"].shape[0], 3)), verbose=False)
    bare = gficf_amd.runReductionSparse({"gficf": data["gficf"]}, reduction=reduction, seed=SEED, ret_model_pred=False, verbose=False, **KW[reduction])
    assert "uwot" not in bare and np.array_equal(np.asarray(bare["embedded"]), emb)


def test_tsne_form_equals_its_stages_and_keeps_the_groups(planted):
    data, labels = planted
    M = data["gficf"]
    out = gficf_amd.runReductionSparse({"gficf": M}, reduction="tsne", seed=SEED, verbose=False, ret_P=True, ret_nn=True, **KW["tsne"])
    nn = gficf_amd.find_nn_sparse(M, 31, True, "euclidean")
    # Rtsne's normalize_input moves no distance but by one factor, the largest magnitude of the gene-centred cells: a stored entry
    # less its gene's mean, or the mean itself where a cell does not store the gene
    mean = np.asarray(M.sum(axis=1)).ravel() / 600
    top = max(np.abs(M.data - mean[M.indices]).max(), np.abs(mean[np.bincount(M.indices, minlength=M.shape[0]) < 600]).max())
    D = np.asarray(M.T.todense())
    assert abs(top / np.abs(D - D.mean(axis=0)).max() - 1) < 1e-12
    dist = nn["dist"] / top
    P = gficf_amd.tsne_affinities(nn["idx"], dist, 10)[0]
    Y0 = np.random.default_rng(SEED).standard_normal((600, 2)) * 1e-4
    Y, kl = gficf_amd.tsne_layout(P, Y0, 150, ret_kl=True)
    emb = np.asarray(out["embedded"])
    assert np.array_equal(emb, Y.astype(np.float64)) and out["reduction"] == "tsne" and out["uwot"] is None
    ts = out["tsne"]
    assert ts["costs"] == kl and ts["space"] == "gficf" and ts["perplexity"] == 10 and ts["max_iter"] == 150 and ts["stop_lying_iter"] == 250
    assert np.array_equal(ts["nn"]["idx"], nn["idx"]) and np.array_equal(ts["nn"]["dist"], dist) and (ts["P"] != P).nnz == 0
    share = _own_share(emb, labels)
    print(f"tsne: own-group share of the 10 nearest neighbours in the plane {share:.4f}")
    assert share >= PURITY["tsne"]
    out = gficf_amd.clustcells(out, from_embedded=True, verbose=False)
    assert len(out["community"]) == 600
    with pytest.raises(NotImplementedError):
        gficf_amd.embedNewCells(out, sp.csc_matrix((M.shape[0], 3)), verbose=False)


def test_inits(planted):
    data, labels = planted
    M = data["gficf"]
    nn = gficf_amd.find_nn_sparse(M, 15, True, "euclidean")
    P = gficf_amd.fuzzy_simplicial_set(nn["idx"], nn["dist"], 1.0, 1.0)[0]
    cells = gficf_amd.rsvd(M, k=2, centre=True)["cells"]
    given = np.random.default_rng(2).uniform(-5, 5, (600, 2))
    starts = {"pca": gficf_amd.umap_init("pca", cells, 600, SEED), "random": gficf_amd.umap_init("random", None, 600, SEED), "array": given}
    for name, Y0 in starts.items():
        with warnings.catch_warnings():
            warnings.simplefilter("error")                               # none of these looks at the graph's components
            out = gficf_amd.runReductionSparse({"gficf": M}, seed=SEED, n_epochs=30, init=given if name == "array" else name, verbose=False)
        want = gficf_amd.umap_layout(P, Y0, 30, 1.0, 1.0, 1.0, 5, 1.0, seed=SEED)
        assert np.array_equal(np.asarray(out["embedded"]), want.astype(np.float64)), name
    with pytest.raises(ValueError, match="init must be"):
        gficf_amd.runReductionSparse({"gficf": M}, init="lvrandom", verbose=False)
    out = gficf_amd.runReductionSparse({"gficf": M}, seed=SEED, n_epochs=30, metric="cosine", init="pca", verbose=False)
    assert out["uwot"]["metric"] == "cosine" and np.isfinite(np.asarray(out["embedded"])).all()


def test_spectral_starts_on_a_connected_graph():
    """Groups of 100 cells and 110 neighbours: every cell names cells of another group, the graph is connected, and the default
    start is the spectral one (and "normlaplacian" the same without scaling and noise), with no warning."""
    counts, labels = _groups(per=100, seed=3)
    M = gficf_amd.gficf(counts, normalize=False, verbose=False)["gficf"]
    nn, P, Y, n_comp = _by_hand_umap(M, "tumap", SEED, 30, k=110)
    assert n_comp == 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = gficf_amd.runReductionSparse({"gficf": M}, seed=SEED, n_neighbors=110, n_epochs=30, verbose=False)
        raw = gficf_amd.runReductionSparse({"gficf": M}, seed=SEED, n_neighbors=110, n_epochs=30, init="normlaplacian", verbose=False)
    assert np.array_equal(np.asarray(out["embedded"]), Y.astype(np.float64))
    want = gficf_amd.umap_layout(P, gficf_amd.spectral_init(P, seed=SEED, jitter=False), 30, 1.0, 1.0, 1.0, 5, 1.0, seed=SEED)
    assert np.array_equal(np.asarray(raw["embedded"]), want.astype(np.float64)) and not np.array_equal(want, Y)


def test_two_components_warn_and_start_from_pca():
    counts, _ = _groups(n_groups=2, per=150, stray=0, seed=4)
    data = gficf_amd.gficf(counts, normalize=False, verbose=False)
    M = data["gficf"]
    with pytest.warns(UserWarning, match=r"more than one component \(2\)"):
        out = gficf_amd.runReductionSparse({"gficf": M}, seed=SEED, n_neighbors=5, n_epochs=30, verbose=False)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        want = gficf_amd.runReductionSparse({"gficf": M}, seed=SEED, n_neighbors=5, n_epochs=30, init="pca", verbose=False)
    assert np.array_equal(np.asarray(out["embedded"]), np.asarray(want["embedded"]))
