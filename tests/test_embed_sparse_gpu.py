"""New cells without PCA on the device: umap_transform_sparse equals its four stages called by hand, bit for bit; a batch may be
cut; embedNewCellsSparse keeps the books of embedNewCells; the new cells land among their own group; classify_cells(method="gficf")
labels them.

Data: the planted groups of tests/test_reduction_sparse_gpu.py, 250 cells per group over 900 genes.  The first 200 of each group
train (gficf, then runReductionSparse: t-UMAP, 100 sweeps, seed 11); the last 50 of each are new, passed as raw counts with all
900 rows.  Statistic: the share of a new cell's 15 nearest TRAINED cells in the plane that carry its label; threshold 0.99, the
project's figure for this data (tests/test_reduction_sparse_gpu.py) and for the hold-out of tests/test_transform_gpu.py."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import gficf_amd
from tests.helpers import sparse_query_oracle as qo
from tests.test_reduction_sparse_gpu import _groups

pytestmark = pytest.mark.gpu

SEED, PER, TRAINED = 11, 250, 200
PURITY = 0.99


@pytest.fixture(scope="module")
def world():
    counts, labels = _groups(per=PER)
    col = np.arange(3 * PER)
    old, new = col[col % PER < TRAINED], col[col % PER >= TRAINED]
    data = gficf_amd.gficf(sp.csc_matrix(counts[:, old]), normalize=False, verbose=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                        # three groups, three components: the start falls back to "pca"
        data = gficf_amd.runReductionSparse(data, reduction="tumap", n_epochs=100, seed=SEED, verbose=False)
    assert data["gficf"].shape[1] == 600 and data["uwot"]["space"] == "gficf"
    x = sp.csc_matrix(counts[:, new])
    assert x.shape == (900, 150)
    sub = x[np.asarray(data["genes"]), :]
    g, kept = gficf_amd.gficf_with_weights(sub, data["w"])
    g = sp.csc_matrix((g.data, kept[g.indices].astype(np.int32), g.indptr), shape=(len(data["w"]), 150))
    return {"data": data, "x": x, "g": g, "old": labels[old], "new": labels[new]}


def _own_share(Y_new, Y_old, lab_new, lab_old, k=15):
    D = ((np.asarray(Y_new)[:, None, :] - np.asarray(Y_old)[None, :, :]) ** 2).sum(-1)
    nn = np.argsort(D, axis=1, kind="stable")[:, :k]
    return float((lab_old[nn] == lab_new[:, None]).mean())


def _by_hand(g, model, train, Y0=None):
    """The four stages through HipOps, one after the other."""
    import torch

    dev, ops = "cuda:0", gficf_amd.HipOps(0)
    G, N = train.shape
    M, k = g.shape[1], int(model["n_neighbors"])
    up = lambda A: [torch.from_numpy(v).to(dev) for v in (A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.astype(np.float64))]
    sws = torch.empty(ops.sparse_query_workspace_bytes(G, N, train.nnz, M, g.nnz, k), dtype=torch.uint8, device=dev)
    idx = torch.empty((k, M), dtype=torch.int32, device=dev)
    dist = torch.empty((k, M), dtype=torch.float32, device=dev)
    ops.sparse_query(G, N, *up(train), M, *up(g), k, model["metric"], sws, idx, None, dist)
    ops.sparse_query_sync(sws)
    w = torch.empty((k, M), dtype=torch.float32, device=dev)
    sigma, rho = (torch.empty(M, dtype=torch.float32, device=dev) for _ in range(2))
    wws, iws, lws = (torch.empty(ops.transform_workspace_bytes(s, M, k=k), dtype=torch.uint8, device=dev) for s in ("weights", "init", "layout"))
    ops.transform_weights(idx, dist, N, M, k, wws, w, 1.0, sigma, rho)
    ops.transform_sync(wws)
    Yt = torch.from_numpy(np.ascontiguousarray(model["embedding"], dtype=np.float32)).to(dev)
    Y = torch.empty((M, 2), dtype=torch.float32, device=dev)
    if Y0 is None:
        ops.transform_init(idx, w, Yt, N, M, k, iws, Y)
        ops.transform_sync(iws)
    else:
        Y.copy_(torch.from_numpy(np.ascontiguousarray(Y0, dtype=np.float32)))
    start = Y.cpu().numpy()
    n_epochs = max(1, int(round(model["n_epochs"] / 3)))
    ops.transform_layout(idx, w, Yt, N, M, k, model["a"], model["b"], 1.0, 0.25, 5, n_epochs, 0, n_epochs, model["seed"], 0, Y, lws)
    ops.transform_sync(lws)
    host = lambda a: np.ascontiguousarray(a.cpu().numpy().T)
    return {"embedding": Y.cpu().numpy().astype(np.float64), "idx": host(idx), "dist": host(dist), "w": host(w), "sigma": sigma.cpu().numpy(),
            "rho": rho.cpu().numpy(), "init": start.astype(np.float64)}


def _equal(a, b):
    assert set(a) == set(b) == {"embedding", "idx", "dist", "w", "sigma", "rho", "init"}
    for key in a:
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), key


def test_transform_equals_its_stages_by_hand(world):
    data, g = world["data"], world["g"]
    got = gficf_amd.umap_transform_sparse(g, data["uwot"], data["gficf"], ret_extra=True)
    assert got["idx"].shape == (150, 15) and got["idx"].dtype == np.int32 and got["dist"].dtype == np.float32 and got["embedding"].dtype == np.float64
    assert got["idx"].min() >= 1 and got["idx"].max() <= 600 and np.isfinite(got["embedding"]).all()
    _equal(got, _by_hand(g, data["uwot"], data["gficf"]))
    nn = gficf_amd.find_nn_sparse_query(data["gficf"], g, 15)                                  # the f32 distances are the search's
    assert np.array_equal(got["idx"], nn["idx"]) and np.array_equal(got["dist"].astype(np.float64), nn["dist"])
    assert np.array_equal(gficf_amd.umap_transform_sparse(g, data["uwot"], data["gficf"]), got["embedding"])


def test_two_halves_with_query_offset_give_the_whole(world):
    data, g = world["data"], world["g"]
    whole = gficf_amd.umap_transform_sparse(g, data["uwot"], data["gficf"], ret_extra=True)
    a = 75
    head = gficf_amd.umap_transform_sparse(sp.csc_matrix(g[:, :a]), data["uwot"], data["gficf"], ret_extra=True)
    tail = gficf_amd.umap_transform_sparse(sp.csc_matrix(g[:, a:]), data["uwot"], data["gficf"], query_offset=a, ret_extra=True)
    _equal({key: np.concatenate([head[key], tail[key]]) for key in whole}, whole)
    shifted = gficf_amd.umap_transform_sparse(sp.csc_matrix(g[:, a:]), data["uwot"], data["gficf"])
    assert not np.array_equal(shifted, whole["embedding"][a:])                                 # the offset is what makes it so


def test_an_init_array_is_honoured(world):
    data, g = world["data"], world["g"]
    Y0 = np.random.default_rng(3).uniform(-3, 3, (150, 2))
    got = gficf_amd.umap_transform_sparse(g, data["uwot"], data["gficf"], init=Y0, ret_extra=True)
    assert np.array_equal(got["init"], Y0.astype(np.float32).astype(np.float64))
    _equal(got, _by_hand(g, data["uwot"], data["gficf"], Y0))
    assert not np.array_equal(got["embedding"], gficf_amd.umap_transform_sparse(g, data["uwot"], data["gficf"]))


def test_embed_new_cells_sparse_books_and_quality(world):
    import pandas as pd

    data, x, g = dict(world["data"]), world["x"], world["g"]
    trained = np.asarray(data["embedded"][["X", "Y"]], dtype=np.float64)
    out = gficf_amd.embedNewCellsSparse(data, x, verbose=False)
    emb = out["embedded"]
    assert len(emb) == 750 and list(emb.columns) == ["X", "Y", "predicted"]
    assert isinstance(emb["predicted"].dtype, pd.CategoricalDtype) and list(emb["predicted"].cat.categories) == ["NO", "YES"]
    assert (emb["predicted"][:600] == "NO").all() and (emb["predicted"][600:] == "YES").all()
    assert np.array_equal(np.asarray(emb[["X", "Y"]])[:600], trained)
    pred = out["gficf.pred"]
    assert sp.isspmatrix_csc(pred) and pred.shape == (len(data["w"]), 150) and (pred != g).nnz == 0
    assert np.array_equal(pred.indptr, g.indptr) and np.array_equal(pred.indices, g.indices) and np.array_equal(pred.data, g.data)
    extra = gficf_amd.umap_transform_sparse(g, data["uwot"], data["gficf"], ret_extra=True)
    new_xy = np.asarray(emb[["X", "Y"]], dtype=np.float64)[600:]
    assert np.array_equal(new_xy, extra["embedding"]) and np.isfinite(new_xy).all()
    before = _own_share(extra["init"], trained, world["new"], world["old"])
    after = _own_share(new_xy, trained, world["new"], world["old"])
    print(f"own-label share of a new cell's 15 nearest trained cells in the plane: {before:.4f} before the sweeps, {after:.4f} after")
    assert after >= PURITY
    # the keywords go to umap_transform_sparse; genes= selects the rows of x by hand
    fewer = gficf_amd.embedNewCellsSparse(dict(world["data"]), x, verbose=False, n_epochs=5, genes=np.asarray(data["genes"]))
    want = gficf_amd.umap_transform_sparse(g, data["uwot"], data["gficf"], n_epochs=5)
    assert np.array_equal(np.asarray(fewer["embedded"][["X", "Y"]], dtype=np.float64)[600:], want)
    with pytest.raises(NotImplementedError, match="embedNewCellsSparse"):
        gficf_amd.embedNewCells(dict(world["data"]), x, verbose=False)


def test_classify_cells_from_the_sparse_columns(world):
    data, x = dict(world["data"]), world["x"]
    out = gficf_amd.embedNewCellsSparse(data, x, verbose=False)
    # the oracle on the device's own GF-ICF output: at least 5 of every new cell's 7 nearest training cells are of its group (a NumPy
    # GF-ICF of this data gave a minimum of 6 of 7 under euclidean), so the vote is decided whatever the order among them
    want = qo.oracle(out["gficf"], out["gficf.pred"], "euclidean", 7)
    own = (world["old"][want["idx"] - 1] == world["new"][:, None]).sum(axis=1)
    print(f"oracle: the fewest of a new cell's 7 nearest training cells in its own group: {own.min()}")
    assert own.min() >= 5
    res = gficf_amd.classify_cells(out, world["old"].astype(str), k=7, method="gficf")
    assert list(res.columns) == ["cell.id", "pred"] and list(res["cell.id"]) == list(range(600, 750))
    assert np.array_equal(np.asarray(res["pred"]), world["new"].astype(str))
    direct = gficf_amd.knn_classify_sparse(out["gficf"], out["gficf.pred"], world["old"], 7)
    assert direct.dtype == world["old"].dtype and np.array_equal(direct, world["new"])
    with pytest.raises(ValueError, match="method must be one of"):
        gficf_amd.classify_cells(out, world["old"].astype(str), method="sparse")
