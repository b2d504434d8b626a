"""libgficf_gsva.so on the GPU against the NumPy oracle of tests/helpers/gsva_np.py: the densities within a measured tolerance,
the order and the walk bit for bit from the device's own densities, the whole call bit for bit on data whose densities are
well apart, reproducibility, relabelled clusters, runGSVA and the deferred rejections."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import gficf_amd
from gficf_amd import GficfError, _gsva_lib
from tests.helpers import gsva_np

pytestmark = pytest.mark.gpu

# Densities: |device - oracle| / max(|oracle|, 1) (d = logit L crosses zero, so small |d| are measured absolutely).  Measured on
# the MI355X over density_case(): 5.507e-14 for d_nz, 1.776e-15 for d0 and, relative, 9.575e-15 for sd (the device's erfc and log
# against libm's, and sums of up to 1025 terms in another order).  Ten times the measured figure is allowed.
DENSITY_MEASURED = 5.507e-14
DENSITY_TOL = 10 * DENSITY_MEASURED
SD_MEASURED = 9.575e-15
SD_TOL = 10 * SD_MEASURED


def density_err(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0))) if len(np.atleast_1d(want)) else 0.0


# ------------------------------------------------------------------ densities
SEG_SIZES = (1, 2, 3, _gsva_lib.TILE - 1, _gsva_lib.TILE, _gsva_lib.TILE + 1, _gsva_lib.JSPLIT - 1, _gsva_lib.JSPLIT, _gsva_lib.JSPLIT + 1)


@functools.lru_cache(maxsize=None)
def density_case():
    """40 genes; one cluster per size of SEG_SIZES, their cells interleaved.  Rows 0 .. 5: no entry at all, an entry in every
    cell (segments of exactly the sizes above), one non-zero value everywhere, stored zeros among the entries, negative values
    among zeros, negative values everywhere; the rest lognormal at densities from 0.2 to 0.95."""
    rng = np.random.default_rng(20241)
    cluster = rng.permutation(np.repeat(np.arange(len(SEG_SIZES)), SEG_SIZES)).astype(np.int32)
    N, G = len(cluster), 40
    X = rng.lognormal(0.0, 1.0, (G, N))
    stored = rng.random((G, N)) < np.linspace(0.2, 0.95, G)[:, None]
    stored[0], stored[1], stored[2], stored[5] = False, True, True, True
    X[2] = 0.75
    X[4] *= rng.choice([-1.0, 1.0], N)
    X[5] = rng.normal(0.0, 2.0, N)
    X[3, rng.random(N) < 0.3] = 0.0                                      # zeros that stay stored
    X = np.where(stored, X, 0.0)
    M = sp.csr_matrix((X[stored], np.nonzero(stored)[1], np.concatenate([[0], np.cumsum(stored.sum(axis=1))])), shape=(G, N))
    assert M.nnz == stored.sum() and (M.data == 0).any()
    sd, kept, D = gsva_np.densities(X, cluster, len(SEG_SIZES))
    return M, X, stored, cluster, sd, kept, D


def test_densities_against_the_oracle():
    M, X, stored, cluster, sd, kept, D = density_case()
    C = len(SEG_SIZES)
    r = gficf_amd.gsva(M, cluster, [0, 3], [1, 4, 5], ret_stages=True, n_clusters=C)
    assert np.array_equal(r["kept"], kept)
    assert not kept[0].any() and not kept[2].any() and not kept[:, 0].any() and kept[1, 1:].all()
    for c, n in enumerate(SEG_SIZES):                                    # the segments of row 1 have the sizes that matter
        assert M[1, np.flatnonzero(cluster == c)].nnz == n
    err_sd = float(np.max(np.abs(r["sd"] - sd) / np.maximum(sd, 1e-300)))
    want_nz = D[stored]                                                  # CSR order: rows, then ascending cells
    err_nz = density_err(r["d_nz"], want_nz)
    # d0 of a (gene, cluster): the oracle's density of any cell of the cluster that does not store the gene
    err_0, seen = 0.0, 0
    for c in range(C):
        cells = np.flatnonzero(cluster == c)
        for g in range(M.shape[0]):
            free = cells[~stored[g, cells]]
            if kept[g, c] and len(free):
                err_0 = max(err_0, density_err(r["d0"][g, c], D[g, free[0]]))
                seen += 1
            elif not kept[g, c] or not len(free):
                assert r["d0"][g, c] == 0.0
    print(f"gsva densities: max err d_nz {err_nz:.3e}, d0 {err_0:.3e} over {seen} segments, sd {err_sd:.3e} (tolerance {DENSITY_TOL:.1e})")
    assert seen > 100 and np.isfinite(r["d_nz"]).all() and (r["d_nz"][~kept[:, cluster][stored]] == 0).all()
    assert err_sd <= SD_TOL and err_nz <= DENSITY_TOL and err_0 <= DENSITY_TOL


# ------------------------------------------------------------------ order and walk, bit for bit
@functools.lru_cache(maxsize=None)
def walk_data():
    """300 genes, clusters of 1, 17 and 300 cells.  Row 0 has no entry; rows 20 .. 24 and 26 none in the cluster of 17 (G_c = 293,
    odd), row 25 none in the cluster of 300 (G_c = 298, even); rows 10 and 11 are identical."""
    rng = np.random.default_rng(77)
    G = 300
    cluster = rng.permutation(np.repeat(np.arange(3), (1, 17, 300))).astype(np.int32)
    N = len(cluster)
    X = rng.lognormal(0.0, 1.0, (G, N)) * (rng.random((G, N)) < 0.5)
    X[0] = 0.0
    X[np.ix_([20, 21, 22, 23, 24, 26], np.flatnonzero(cluster == 1))] = 0.0
    X[25, cluster == 2] = 0.0
    X[11] = X[10]
    M = sp.csr_matrix(X)
    sets = [[7], [8], [9], [40], [41], [150],                            # m = 1
            [g for g in range(G) if g != 5],                             # m = G_c - 1 in both clusters
            [20, 21, 22, 23, 24, 30, 31],                                # 2 of its 7 members are kept in the cluster of 17
            [10, 11, 12], [10, 200], [11, 201]]
    sets += [list(range(30, 30 + m)) for m in (31, 32, 33, 63, 64, 65, 255, 256, 257)]
    ptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    return M, cluster, ptr, np.concatenate(sets).astype(np.int32)


@functools.lru_cache(maxsize=None)
def walk_case():
    """walk_data() and the device's own stage outputs on it."""
    M, cluster, ptr, members = walk_data()
    return M, cluster, ptr, members, gficf_amd.gsva(M, cluster, ptr, members, ret_stages=True, n_clusters=3)


def seq_sums(es, cluster, C):
    """Per (row, cluster) the sum over the cluster's cells in ascending order, one addition each, and the same of the squares."""
    out = np.zeros((2, es.shape[0], C))
    for c in range(C):
        sub = es[:, cluster == c]
        if sub.shape[1]:
            out[0, :, c], out[1, :, c] = np.cumsum(sub, axis=1)[:, -1], np.cumsum(sub * sub, axis=1)[:, -1]
    return out


@pytest.mark.parametrize("min_size,max_size", [(1, np.inf), (3, np.inf), (2, 64)])
def test_order_and_walk_bit_for_bit(min_size, max_size):
    M, cluster, ptr, members, st = walk_case()
    kept = st["kept"]
    assert list(kept.sum(axis=0)) == [0, 293, 298]
    D = gsva_np.dense_densities(M, cluster, st["d_nz"], st["d0"])
    want, tested = gsva_np.scores(D, kept, cluster, 3, ptr, members, min_size, max_size)
    got = gficf_amd.gsva_scores(st["d_nz"], st["d0"], kept, M, cluster, ptr, members, min_size, max_size, n_clusters=3)
    assert np.array_equal(got["tested"], tested) and not tested[:, 0].any()
    np.testing.assert_array_equal(got["es"], want)                      # NaN where the oracle has NaN
    if min_size == 1:
        assert tested[6].tolist() == [False, True, True] and tested[:6, 1:].all()
        assert np.isnan(want[:6, cluster == 2]).any() and not np.isnan(want[:, cluster == 1]).any()     # W = 0 needs an even G_c
        np.testing.assert_array_equal(gficf_amd.gsva(M, cluster, ptr, members, n_clusters=3)["es"], want)   # the one-call form: the same bits
    if min_size == 3:
        assert tested[7].tolist() == [False, False, True] and not tested[:6].any()
    if min_size == 2:
        assert not tested[6].any() and not tested[16:].any() and tested[11:16, 1:].all()
    with np.errstate(invalid="ignore"):
        sums = seq_sums(got["es"], cluster, 3)
    np.testing.assert_array_equal(got["sum"], sums[0])
    np.testing.assert_array_equal(got["sumsq"], sums[1])


def test_long_cells_and_a_mask_beyond_one_word_per_thread():
    # more than 2048 stored entries per cell (the LDS lists at their full 4096 slots, beyond 64 KiB of LDS) and G_c > 8192
    # (more than 256 mask words: a thread of the walker owns three)
    rng = np.random.default_rng(5)
    G = 10500
    cluster = np.array([0, 1, 0, 0, 1, 0, 0, 1], dtype=np.int32)
    X = rng.lognormal(0.0, 1.0, (G, len(cluster))) * (rng.random((G, len(cluster))) < 0.3)
    M = sp.csr_matrix(X)
    assert 2048 < np.diff(M.tocsc().indptr).max() <= _gsva_lib.MAX_CELL_NZ
    sets = [list(rng.permutation(G)[:m]) for m in (1, 40, 700, 5000)] + [list(range(G))]
    ptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    members = np.concatenate(sets).astype(np.int32)
    got = gficf_amd.gsva(M, cluster, ptr, members, ret_stages=True)
    sd, kept = (np.stack(v, axis=1) for v in zip(*(gsva_np.gene_filter(X[:, cluster == c]) for c in range(2))))
    assert np.array_equal(got["kept"], kept) and kept[:, 0].sum() > 8192 > kept[:, 1].sum() > 0
    D = gsva_np.dense_densities(M, cluster, got["d_nz"], got["d0"])
    want, tested = gsva_np.scores(D, kept, cluster, 2, ptr, members)
    assert np.array_equal(got["tested"], tested) and tested[1:4].all() and not tested[4].any()       # every gene: m = G_c, not below it
    np.testing.assert_array_equal(got["es"], want)


# ------------------------------------------------------------------ end to end, independent of the device's densities
@functools.lru_cache(maxsize=None)
def lognormal_case():
    """60 genes at density 0.6 in clusters of 40 and 75 cells, lognormal(0, 0.5).  A value far above the rest of its gene has
    L = 1 - 0.5 / n but for a tail of some 1e-14, the same in every gene, so near-ties of densities are common at sigma = 1;
    this sigma and seed were picked on the CPU for the gap the test asserts first (2.4e-7)."""
    rng = np.random.default_rng(3)
    G, sizes = 60, (40, 75)
    cluster = rng.permutation(np.repeat(np.arange(2), sizes)).astype(np.int32)
    X = rng.lognormal(0.0, 0.5, (G, len(cluster))) * (rng.random((G, len(cluster))) < 0.6)
    sets = [list(rng.permutation(G)[:m]) for m in (5, 9, 17, 30, 45, 59)]
    ptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    return sp.csr_matrix(X), X, cluster, ptr, np.concatenate(sets).astype(np.int32)


def test_whole_call_against_the_numpy_oracle():
    M, X, cluster, ptr, members = lognormal_case()
    ref = gsva_np.gsva_np(X, cluster, 2, ptr, members)
    assert ref["kept"].all() and ref["tested"].all()
    gap = np.inf                                                         # the order of every cell must not hang on the densities' last bits
    for j in range(X.shape[1]):
        d = np.sort(ref["D"][:, j])
        step = np.diff(d)
        gap = min(gap, float(np.min((step / np.maximum(np.abs(d[1:]), 1.0))[step > 0])))
    assert gap > 100 * DENSITY_TOL, gap
    got = gficf_amd.gsva(M, cluster, ptr, members, ret_stages=True)
    assert np.array_equal(got["kept"], ref["kept"]) and np.array_equal(got["tested"], ref["tested"])
    assert density_err(got["d_nz"], ref["D"][X != 0]) <= DENSITY_TOL
    np.testing.assert_array_equal(got["es"], ref["es"])
    assert np.abs(got["es"]).max() <= 1.0


def test_same_input_same_bits_and_relabelled_clusters():
    M, X, cluster, ptr, members = lognormal_case()
    a = gficf_amd.gsva(M, cluster, ptr, members, ret_stages=True, n_clusters=3)
    b = gficf_amd.gsva(M, cluster, ptr, members, ret_stages=True, n_clusters=3)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k
    perm = np.array([2, 0, 1], dtype=np.int32)                           # old id -> new id; the third cluster is empty
    c = gficf_amd.gsva(M.tocsc(), perm[cluster], ptr, members, ret_stages=True, n_clusters=3)
    assert np.array_equal(c["es"], a["es"]) and np.array_equal(c["d_nz"], a["d_nz"])
    for k in ("tested", "kept", "sum", "sumsq", "sd", "d0"):
        assert np.array_equal(c[k][:, perm], a[k]), k
    assert not a["tested"][:, 2].any() and not a["kept"][:, 2].any()


# ------------------------------------------------------------------ runGSVA
def test_run_gsva_on_a_synthetic_analysis():
    rng = np.random.default_rng(11)
    G, N, P = 120, 600, 10
    lab = rng.choice(np.array(["3", "1", "2"]), N, p=[0.5, 0.3, 0.2])
    shift = {"3": 0, "1": 1, "2": 2}
    X = rng.lognormal(0.0, 1.0, (G, N)) * (rng.random((G, N)) < 0.4)
    for k, s in shift.items():                                           # in half of each cluster's cells a block of genes is lifted
        X[np.ix_(np.arange(20 * s, 20 * s + 20), np.flatnonzero((lab == k) & (rng.random(N) < 0.5)))] *= 3.0
    names = np.array([f"g{i}" for i in range(G)])
    pathways = {f"set{p}": list(names[20 * (p % 6):20 * (p % 6) + 20]) + ["unknown"] for p in range(6)}
    pathways.update({f"rand{p}": list(names[rng.permutation(G)[:25]]) for p in range(P - 7)})
    pathways["small"] = list(names[:5])                                  # below minSize: zero everywhere, dropped from res
    data = {"gficf": sp.csc_matrix(X), "cluster": lab, "gene_names": names}
    out = gficf_amd.runGSVA(data, pathways=pathways, verbose=False)["gsva"]
    res, de = out["res"], out["DEpathways"]
    assert set(out) == {"pathways", "res", "DEpathways"} and list(out["pathways"]) == list(pathways)
    assert res.shape == (P - 1, N) and list(res.index) == [k for k in pathways if k != "small"]
    assert list(de.columns) == ["logFC", "AveExpr", "t", "P.Value", "adj.P.Val", "pathway", "cluster"] and len(de) == 3 * (P - 1)
    uniq = list(dict.fromkeys(lab))                                      # unique() order
    assert list(dict.fromkeys(de["cluster"])) == uniq
    ids = np.array([uniq.index(x) for x in lab])
    want = gsva_np.de_pathways(res.to_numpy(), ids, 3)
    assert list(de["pathway"]) == [res.index[i] for i in want["pathway"]] and list(de["cluster"]) == [uniq[c] for c in want["cluster"]]
    for k in ("logFC", "AveExpr", "t", "P.Value", "adj.P.Val"):
        np.testing.assert_allclose(de[k].to_numpy(), want[k], rtol=1e-10, atol=0, err_msg=k)
    assert ((de["P.Value"] > 0) & (de["P.Value"] <= 1) & (de["adj.P.Val"] >= de["P.Value"])).all()
    for lab_c in uniq:                                                   # each cluster's rows by decreasing |t|
        assert (np.diff(np.abs(de[de["cluster"] == lab_c]["t"].to_numpy())) <= 0).all()
    flipped = gficf_amd.runGSVA(dict(data), pathways=pathways, verbose=False, cluster_minus_other=True)["gsva"]["DEpathways"]
    assert np.array_equal(flipped["logFC"].to_numpy(), -de["logFC"].to_numpy()) and np.array_equal(flipped["P.Value"].to_numpy(), de["P.Value"].to_numpy())


# ------------------------------------------------------------------ deferred rejections
def test_deferred_rejections():
    M, X, cluster, ptr, members = lognormal_case()
    bad = M.copy()
    bad.data[7] = np.nan
    with pytest.raises(GficfError, match="NaN or an infinite"):
        gficf_amd.gsva(bad, cluster, ptr, members)
    bad.data[7] = np.inf
    with pytest.raises(GficfError, match="NaN or an infinite"):
        gficf_amd.gsva(bad, cluster, ptr, members)
    twice = members.copy()
    twice[1] = twice[0]
    with pytest.raises(GficfError, match="repeated within a pathway"):
        gficf_amd.gsva(M, cluster, ptr, twice)
    far = members.copy()
    far[3] = M.shape[0]
    with pytest.raises(GficfError, match=r"member outside \[0, G\)"):
        gficf_amd.gsva(M, cluster, ptr, far)
    off = cluster.copy()
    off[5] = -1
    with pytest.raises(GficfError, match=r"cluster id outside \[0, C\)"):
        gficf_amd.gsva(M, off, ptr, members)
    with pytest.raises(GficfError, match=r"cluster id outside \[0, C\)"):
        gficf_amd.gsva(M, cluster, ptr, members, n_clusters=1)
    wide = sp.csr_matrix(np.ones((_gsva_lib.MAX_CELL_NZ + 1, 2)))
    with pytest.raises(GficfError, match="stored entries"):
        gficf_amd.gsva(wide, np.zeros(2, dtype=np.int32), [0, 2], [0, 1])
    good = gficf_amd.gsva(M, cluster, ptr, members)                      # the context is as usable as before
    assert np.isfinite(good["es"]).all()
