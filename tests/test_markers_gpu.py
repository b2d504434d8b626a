"""GPU: the marker-gene test (libgficf_markers.so) against the NumPy oracle of tests/helpers/markers_np.py.
Bar: p within rtol 1e-12 and exactly 1.0 where the oracle gives 1 (U and T are integers on the device, z carries the
reference's arithmetic without fused multiply-adds); log2FC within 1e-10 absolute."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

import gficf_amd
from gficf_amd import GficfError, synth
from gficf_amd import _markers_lib
from gficf_amd.api import _np_ptr, default_context
from tests.helpers import markers_np as mk

pytestmark = pytest.mark.gpu


def _labels(seed, N, C, sizes=None):
    rng = np.random.default_rng(seed)
    if sizes is None:
        ids = np.concatenate([np.arange(C), rng.integers(0, C, N - C)])
    else:
        ids = np.repeat(np.arange(C), sizes)
    rng.shuffle(ids)
    return ids.astype(np.int32)


def _check(P, LFC, labels, ref):
    cols = [int(l) for l in labels]
    rp, rl = ref["p"][:, cols], ref["lfc"][:, cols]
    one = rp == 1.0
    assert np.array_equal(P[one], rp[one])
    assert np.allclose(P[~one], rp[~one], rtol=1e-12, atol=0), np.abs(P / rp - 1).max()
    assert np.abs(LFC - rl).max(initial=0) <= 1e-10


def _csc(colptr, rowidx, x, G, N):
    return sp.csc_matrix((x, rowidx, colptr), shape=(G, N))


def test_raw_counts_heavy_ties_against_the_literal_oracle():
    colptr, rowidx, x = synth.counts_csc(60, 700, median_frac=0.3, seed=11)
    M = _csc(colptr, rowidx, x, 60, 700)
    ids = _labels(1, 700, 5)
    P, LFC, labels = gficf_amd.cluster_markers(M, ids)
    _check(P, LFC, labels, mk.markers_literal(M.toarray(), ids, 5))


@pytest.mark.parametrize("C", [2, 30])
def test_raw_and_cpm_values_against_the_shared_sort_oracle(C):
    G, N = 300, 4000
    colptr, rowidx, x = synth.counts_csc(G, N, seed=12)
    M = _csc(colptr, rowidx, x, G, N)
    ids = _labels(2, N, C)
    for mat in (M, sp.csc_matrix(M.multiply(1e6 / np.asarray(M.sum(0))).tocsc())):
        P, LFC, labels = gficf_amd.cluster_markers(mat, ids)
        _check(P, LFC, labels, mk.markers_shared(mat, ids, C))


def test_negative_values_explicit_zeros_and_negative_zero():
    rng = np.random.default_rng(4)
    G, N, C = 40, 900, 6
    D = rng.poisson(0.7, (G, N)).astype(np.float64)
    D[rng.random((G, N)) < 0.3] *= -1.5
    D[3] = 0.0
    D[4] = 2.5                                            # one distinct value
    M = sp.csc_matrix(D)
    # store explicit zeros and -0.0 next to the non-zeros
    coo = M.tocoo()
    extra_r, extra_c = rng.integers(0, G, 400), rng.integers(0, N, 400)
    free = D[extra_r, extra_c] == 0
    er, ec = extra_r[free], extra_c[free]
    ev = np.where(np.arange(len(er)) % 2 == 0, 0.0, -0.0)
    key = er * N + ec
    _, first = np.unique(key, return_index=True)
    er, ec, ev = er[first], ec[first], ev[first]
    Z = sp.csc_matrix((np.concatenate([coo.data, ev]), (np.concatenate([coo.row, er]), np.concatenate([coo.col, ec]))), shape=(G, N))
    Z.sort_indices()
    assert Z.nnz > M.nnz
    ids = _labels(3, N, C)
    P, LFC, labels = gficf_amd.cluster_markers(Z, ids)
    ref = mk.markers_literal(D, ids, C)
    _check(P, LFC, labels, ref)
    assert (P[3] == 1.0).all() and (P[4] == 1.0).all()


def test_complete_separation_closed_form():
    N, n1 = 500, 120
    ids = np.zeros(N, dtype=np.int32)
    ids[n1:] = 1
    vals = np.concatenate([1000.0 + np.arange(n1), 1.0 + np.arange(N - n1)])    # distinct, non-zero, cluster 0 on top
    M = sp.csc_matrix(vals[None, :])
    P, LFC, labels = gficf_amd.cluster_markers(M, ids)
    n2 = N - n1
    z = (0 - (n1 * n2) // 2 + 0.5) / math.sqrt((n1 * n2 / 12) * ((n1 + n2 + 1) - 0 / ((n1 + n2) * (n1 + n2 - 1))))
    p = math.erfc(abs(z) / math.sqrt(2))
    assert P[0, 0] == pytest.approx(p, rel=1e-12) and P[0, 1] == pytest.approx(p, rel=1e-12)
    s1, s2 = vals[:n1].sum(), vals[n1:].sum()
    assert LFC[0, 0] == pytest.approx(math.log2(((s1 + n1) / n1) / ((s2 + n2) / n2)), abs=1e-10)


def test_200k_cells_gene_dense_with_ties_across_every_chunk():
    N, C = 200_000, 30
    rng = np.random.default_rng(9)
    rows = np.stack([np.where(np.arange(N) % 7 == 0, 2.0, 1.0),              # two tie groups of 171 k and 29 k cells
                     np.full(N, 3.0),                                          # one distinct value
                     rng.permutation(N) + 0.5,                                 # all distinct
                     np.where(rng.random(N) < 0.5, 0.0, rng.integers(1, 4, N).astype(float))])
    M = sp.csc_matrix(rows)
    ids = _labels(5, N, C)
    P, LFC, labels = gficf_amd.cluster_markers(M, ids)
    ref = mk.markers_shared(M, ids, C)
    _check(P, LFC, labels, ref)
    assert (P[1] == 1.0).all()


def test_five_thousand_clusters_with_singletons_global_accumulators():
    G, N, C = 25, 12000, 5000
    colptr, rowidx, x = synth.counts_csc(G, N, median_frac=0.5, seed=13)
    M = _csc(colptr, rowidx, x, G, N)
    sizes = np.ones(C, dtype=np.int64)
    sizes[:50] += (N - C) // 50
    sizes[0] += N - sizes.sum()
    ids = _labels(6, N, C, sizes)
    P, LFC, labels = gficf_amd.cluster_markers(M, ids)
    _check(P, LFC, labels, mk.markers_shared(M, ids, C))


def test_dense_two_matrix_form_equals_csc_and_the_literal_oracle():
    rng = np.random.default_rng(7)
    G, n1, n2 = 50, 130, 410
    X = rng.poisson(1.2, (G, n1)).astype(np.float64)
    Y = rng.poisson(0.9, (G, n2)).astype(np.float64)
    X[0] = 0.0
    Y[0] = 0.0                                            # all zero: p = 1
    out = gficf_amd.rcpp_parallel_WMU_test(X, Y)
    assert out.shape == (G, 2)
    ref = mk.wmu_dense_literal(X, Y)
    one = ref[:, 0] == 1.0
    assert np.array_equal(out[one, 0], ref[one, 0]) and one[0]
    assert np.allclose(out[~one, 0], ref[~one, 0], rtol=1e-12, atol=0)
    assert np.abs(out[:, 1] - ref[:, 1]).max() <= 1e-10
    ids = np.r_[np.zeros(n1, np.int32), np.ones(n2, np.int32)]
    P, LFC, labels = gficf_amd.cluster_markers(sp.csc_matrix(np.hstack([X, Y])), ids)
    assert np.array_equal(P[:, 0], out[:, 0]) and np.array_equal(LFC[:, 0], out[:, 1])
    # rcpp_WMU_test: 1-based column subsets of one matrix
    A = np.hstack([X, Y])
    i1, i2 = np.arange(1, n1 + 1), np.arange(n1 + 1, n1 + n2 + 1)
    assert np.array_equal(gficf_amd.rcpp_WMU_test(A, i1, i2), out)


def test_host_and_device_forms_equal_repeatable_and_permutation_invariant():
    torch = pytest.importorskip("torch")
    G, N, C = 200, 3000, 9
    colptr, rowidx, x = synth.counts_csc(G, N, seed=14)
    M = _csc(colptr, rowidx, x, G, N)
    ids = _labels(8, N, C)
    P, LFC, labels = gficf_amd.cluster_markers(M, ids)
    P2, LFC2, _ = gficf_amd.cluster_markers(M, ids)
    assert np.array_equal(P, P2) and np.array_equal(LFC, LFC2)
    ops = gficf_amd.HipOps(0)
    dev = torch.device("cuda", 0)
    fa, _ = gficf_amd.api._first_appearance_ids(ids, N)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ws = torch.empty(ops.cluster_markers_workspace_bytes(G, N, len(rowidx), C), dtype=torch.uint8, device=dev)
    p = torch.empty((C, G), dtype=torch.float64, device=dev)
    lfc = torch.empty((C, G), dtype=torch.float64, device=dev)
    ops.cluster_markers(G, N, t(colptr.astype(np.int64)), t(rowidx.astype(np.int32)), t(x), t(fa), C, ws, p, lfc)
    ops.cluster_markers_sync(ws)
    assert np.array_equal(p.cpu().numpy().T, P) and np.array_equal(lfc.cpu().numpy().T, LFC)
    perm = np.random.default_rng(1).permutation(N)
    Pp, LFCp, labels_p = gficf_amd.cluster_markers(M[:, perm], ids[perm])
    order = [list(labels_p).index(l) for l in labels]
    assert np.array_equal(Pp[:, order], P)
    assert np.array_equal(LFCp[:, order], LFC)


def test_error_codes():
    L = _markers_lib.load()
    ctx = default_context()
    G, N = 3, 6
    colptr = np.arange(N + 1, dtype=np.int64)
    rowidx = np.array([0, 1, 2, 0, 1, 2], dtype=np.int32)
    x = np.arange(1.0, 7.0)
    p = np.zeros(G * 4)
    l = np.zeros(G * 4)

    def run(x=x, rowidx=rowidx, cl=np.array([0, 1, 0, 1, 0, 1], np.int32), C=2, colptr=colptr):
        return L.gficf_cluster_markers_host(ctx.handle, G, N, _np_ptr(colptr), 1, _np_ptr(rowidx), _np_ptr(x), _np_ptr(cl), C, _np_ptr(p), _np_ptr(l))

    assert run() == 0
    assert run(x=np.where(np.arange(6) == 2, np.nan, x)) == 8                 # GFICF_ERR_BAD_VALUE
    assert run(C=1, cl=np.zeros(N, np.int32)) == 1                           # C < 2
    assert run(C=3) == 1                                                      # cluster 2 empty
    assert run(cl=np.array([0, 1, 0, 1, 0, 2], np.int32)) == 1                # label outside [0, C)
    assert run(rowidx=np.array([0, 1, 2, 0, 7, 2], np.int32)) == 3           # GFICF_ERR_BAD_CSC
    assert run(colptr=np.array([0, 1, 3, 2, 4, 5, 6], np.int64)) == 3
    assert run() == 0                                                         # the context is fine afterwards
    with pytest.raises(GficfError, match="GFICF_ERR_BAD_VALUE"):
        gficf_amd.rcpp_parallel_WMU_test(np.array([[1.0, np.nan]]), np.array([[2.0]]))
    torch = pytest.importorskip("torch")
    ops = gficf_amd.HipOps(0)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ws = torch.empty(ops.cluster_markers_workspace_bytes(G, N, N, 2), dtype=torch.uint8, device=dev)
    pp = torch.empty((2, G), dtype=torch.float64, device=dev)
    ll = torch.empty((2, G), dtype=torch.float64, device=dev)
    ops.cluster_markers(G, N, t(colptr), t(rowidx), t(x), t(np.array([0, 1, 0, 1, 0, 5], np.int32)), 2, ws, pp, ll)
    with pytest.raises(GficfError, match="GFICF_ERR_INVALID_ARG"):
        ops.cluster_markers_sync(ws)


def test_find_cluster_markers_end_to_end():
    G, N = 150, 2500
    colptr, rowidx, x = synth.counts_csc(G + 10, N, seed=15)
    raw = _csc(colptr, rowidx, x, G + 10, N).tolil()
    raw[G:, :] = 0                                        # genes without a non-zero cell: dropped before the test (BH's n)
    raw = sp.csc_matrix(raw)
    raw.eliminate_zeros()
    ids = _labels(10, N, 6)
    D = raw.toarray()
    boost = ids == 3
    D[:20][:, boost] += 4.0                               # markers of cluster 3
    cpms = sp.csc_matrix(D / np.maximum(D.sum(0), 1.0) * 1e6)
    data = {"community": ids + 1, "cluster": (ids + 1).astype(str), "rawCounts": raw, "genes": np.arange(G + 10) + 1000}
    out = gficf_amd.findClusterMarkers(data, hvg=False, verbose=False, cpms=cpms)
    df = out["de.genes"]
    assert list(df.columns) == ["ens", "log2FC", "p.value", "fdr", "cluster"]
    kept = np.flatnonzero(np.asarray((cpms != 0).sum(1)).ravel() > 0)
    assert len(kept) == G
    labels = list(dict.fromkeys((ids + 1).astype(str)))
    fa = np.array([labels.index(s) for s in (ids + 1).astype(str)])
    ref = mk.markers_shared(cpms[kept], fa, len(labels))
    want = mk.find_cluster_markers(ref["p"], ref["lfc"], labels, kept + 1000)
    assert len(df) == len(want) and len(want) > 10
    assert list(df["ens"]) == [r[0] for r in want] and list(df["cluster"]) == [r[4] for r in want]
    assert np.allclose(df["log2FC"], [r[1] for r in want], rtol=0, atol=1e-10)
    assert np.allclose(df["p.value"], [r[2] for r in want], rtol=1e-12, atol=0)
    assert np.allclose(df["fdr"], [r[3] for r in want], rtol=1e-12, atol=0)
    assert (df.loc[df["cluster"] == labels[fa[boost][0]], "ens"] < 1020).any()
    with pytest.warns(UserWarning, match="raw counts"):
        gficf_amd.findClusterMarkers(dict(data), hvg=False, verbose=False)


# ------------------------------------------------------------------------------------------------ at scale and at every switch point
def _config3_like(G, N, nnz, seed):
    """genes x cells CPM matrix with about nnz stored entries (Zipf-like gene popularity, counts 1 + geometric)."""
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, G + 1) ** 0.6
    gene = rng.choice(G, nnz, p=w / w.sum())
    cell = rng.integers(0, N, nnz)
    lin = np.unique(cell.astype(np.int64) * G + gene)
    c, g = lin // G, (lin % G).astype(np.int32)
    cnt = (1 + rng.geometric(0.5, len(lin))).astype(np.float64)
    colsum = np.bincount(c, weights=cnt, minlength=N)
    x = cnt / colsum[c] * 1e6
    colptr = np.concatenate([[0], np.cumsum(np.bincount(c, minlength=N))]).astype(np.int64)
    return sp.csc_matrix((x, g, colptr), shape=(G, N))


def _uneven_labels(seed, N, C):
    rng = np.random.default_rng(seed)
    w = rng.pareto(1.2, C) + 0.05
    sizes = np.maximum(1, np.floor(w / w.sum() * (N - C))).astype(np.int64) + 0
    sizes[np.argmax(sizes)] += N - sizes.sum()
    return _labels(seed, N, C, sizes)


@pytest.fixture(scope="module")
def config3():
    return _config3_like(23_000, 54_000, 10_800_000, seed=31)


def test_config3_scale_ten_million_entries(config3):
    """23 k genes (plain transpose, one gene range), 54 k cells, 45 uneven clusters: the three b = 32 / 15-bit sorts walk
    several tiles per workgroup and the gene sort takes two passes."""
    M = config3
    assert M.nnz >= 10_000_000
    ids = _uneven_labels(32, M.shape[1], 45)
    P, LFC, labels = gficf_amd.cluster_markers(M, ids)
    _check(P, LFC, labels, mk.markers_sparse(M, ids, 45))


@pytest.mark.parametrize("C", [2048, 2049])
def test_lds_and_global_accumulators_at_the_switch(config3, C):
    """C = 2048: 64 KiB of LDS accumulators (+ 48 B) a workgroup; 2049: global ones.  G * C > 16384 * 256: the epilogue
    grid-strides."""
    M = config3[:2600]
    assert M.shape[0] * C > 16384 * 256
    ids = _uneven_labels(33, M.shape[1], C)
    P, LFC, labels = gficf_amd.cluster_markers(M, ids)
    _check(P, LFC, labels, mk.markers_sparse(M, ids, C))


def test_million_genes_walk_grid_strides():
    """1.1 M genes x 64 cells: a 21-bit gene sort in three passes, more genes than walk workgroups (2^20), 30 gene ranges of
    the transpose."""
    G, N = 1_100_000, 64
    rng = np.random.default_rng(34)
    nnz = 3_000_000
    M = sp.csc_matrix((rng.integers(1, 6, nnz).astype(np.float64) * 0.5, (rng.integers(0, G, nnz), rng.integers(0, N, nnz))), shape=(G, N))
    M.sum_duplicates()
    ids = _labels(35, N, 3)
    P, LFC, labels = gficf_amd.cluster_markers(M, ids)
    _check(P, LFC, labels, mk.markers_sparse(M, ids, 3))


MK_MAX_N = 2_097_151


def test_largest_n_tie_sums_near_two_to_the_63():
    N = MK_MAX_N
    rng = np.random.default_rng(36)
    rows = np.zeros((4, N))
    rows[0] = 7.25                                        # one tie group of N - 4 cells: t^3 - t close to 2^63
    rows[0, [11, 500, N - 3, N - 1]] = [0.0, 1.0, 9.0, -2.0]
    rows[1, rng.choice(N, 3, replace=False)] = [4.0, 4.0, -1.0]      # nearly all zero: Z^3 - Z close to 2^63
    rows[2] = rng.permutation(N) + 0.5                    # all distinct
    rows[3] = np.where(rng.random(N) < 0.4, 1.5, 3.0)     # two tie groups
    M = sp.csc_matrix(rows)
    ids = np.zeros(N, dtype=np.int32)
    ids[rng.integers(0, N)] = 1                           # a cluster of one cell: n1 * n2 odd
    P, LFC, labels = gficf_amd.cluster_markers(M, ids)
    ref = mk.markers_sparse(M, ids, 2)
    assert ref["T"][0, 0] > 2 ** 62 and ref["T"][1, 0] > 2 ** 62
    _check(P, LFC, labels, ref)


def test_one_cell_more_than_the_largest_n_is_rejected_before_allocating():
    L = _markers_lib.load()
    N = MK_MAX_N + 1
    ctx = gficf_amd.api.Context(0)                        # empty pools: an allocation would show in the free memory
    try:
        torch = pytest.importorskip("torch")
        colptr = np.zeros(N + 1, dtype=np.int64)
        cl = (np.arange(N) % 2).astype(np.int32)
        p, l = np.zeros(2), np.zeros(2)
        free0 = torch.cuda.mem_get_info(0)[0]
        rc = L.gficf_cluster_markers_host(ctx.handle, 1, N, _np_ptr(colptr), 1, None, None, _np_ptr(cl), 2, _np_ptr(p), _np_ptr(l))
        assert rc == 6                                    # GFICF_ERR_UNSUPPORTED
        X, Y = np.zeros((1, N // 2)), np.zeros((1, N - N // 2))
        out = np.zeros(2)
        assert L.gficf_cluster_markers_dense_host(ctx.handle, 1, X.shape[1], _np_ptr(X), Y.shape[1], _np_ptr(Y), _np_ptr(out)) == 6
        assert free0 - torch.cuda.mem_get_info(0)[0] < 4 << 20
        assert L.gficf_cluster_markers_workspace_bytes(1, N, 0, 2) > 0
    finally:
        ctx.close()


# values far outside expression data: a single huge (or tiny) cell next to fractional values
RANGE_SPIKES = [1e20, -1e20, 1e25, 1e30, 1e40, 1e300, 1e-300, 5e-324]


def _range_matrix(N, seed, density):
    rng = np.random.default_rng(seed)
    G = len(RANGE_SPIKES) + 1
    D = np.where(rng.random((G, N)) < density, rng.random((G, N)) * 3, 0.0)
    for g, v in enumerate(RANGE_SPIKES):
        D[g, rng.integers(0, N)] = v
    D[-1, rng.integers(0, N)] = 1e30                      # with 1e-300 and 5e-324 in the same gene
    D[-1, rng.integers(0, N)] = 1e-300
    D[-1, rng.integers(0, N)] = 5e-324
    return D


def _check_range(P, LFC, labels, ref):
    cols = [int(l) for l in labels]
    rl = ref["lfc"][:, cols]
    nan = np.isnan(rl)
    assert np.array_equal(np.isnan(LFC), nan)
    err = np.abs(LFC[~nan] - rl[~nan])
    assert err.max(initial=0) <= 1e-10, err.max()
    _check(P, np.where(nan, 0.0, LFC), labels, {"p": ref["p"], "lfc": np.where(np.isnan(ref["lfc"]), 0.0, ref["lfc"])})


def test_log2fc_over_the_whole_double_range_small_n():
    N, C = 2000, 5
    D = _range_matrix(N, 37, 0.5)
    ids = _labels(38, N, C)
    M = sp.csc_matrix(D)
    P, LFC, labels = gficf_amd.cluster_markers(M, ids)
    ref = mk.markers_sparse(M, ids, C)
    pos = [g for g, v in enumerate(RANGE_SPIKES + [1.0]) if v > 0]   # (the -1e20 gene: log2 of a negative ratio, NaN everywhere)
    lit = mk.markers_literal(D[pos], ids, C)
    for k in ("p", "lfc"):
        ref[k][pos] = lit[k]
    assert np.isnan(ref["lfc"][RANGE_SPIKES.index(-1e20)]).all()
    _check_range(P, LFC, labels, ref)
    P2, LFC2, _ = gficf_amd.cluster_markers(M, ids)                  # repeatable, and invariant under a permutation of the cells
    assert np.array_equal(P, P2) and np.array_equal(LFC, LFC2, equal_nan=True)
    perm = np.random.default_rng(39).permutation(N)
    Pp, LFCp, labels_p = gficf_amd.cluster_markers(M[:, perm], ids[perm])
    order = [list(labels_p).index(l) for l in labels]
    assert np.array_equal(Pp[:, order], P) and np.array_equal(LFCp[:, order], LFC, equal_nan=True)
    # the dense two-matrix form once
    inn = ids == 0
    out = gficf_amd.rcpp_parallel_WMU_test(D[pos][:, inn], D[pos][:, ~inn])
    ref = mk.wmu_dense_literal(D[pos][:, inn], D[pos][:, ~inn])
    assert np.abs(out[:, 1] - ref[:, 1]).max() <= 1e-10
    assert np.allclose(out[:, 0], ref[:, 0], rtol=1e-12, atol=0)


def test_log2fc_over_the_whole_double_range_two_million_cells():
    """N near 2^21 moves the fixed-point window about ten bits lower.  The reference's sums there: exact ones (fsum) of the
    cluster's and the rest's values, which its running f64 sums match far inside the 1e-10 bar."""
    N, C = 2_000_000, 3
    rng = np.random.default_rng(40)
    G = len(RANGE_SPIKES) + 1
    rows, cols, vals = [], [], []
    for g in range(G):
        c = np.unique(rng.integers(0, N, 60_000))
        v = rng.random(len(c)) * 3
        spikes = [RANGE_SPIKES[g]] if g < len(RANGE_SPIKES) else [1e30, 1e-300, 5e-324]
        at = rng.choice(np.setdiff1d(np.arange(1000), c), len(spikes), replace=False)
        rows += [np.full(len(c) + len(at), g)]
        cols += [c, at]
        vals += [v, np.array(spikes)]
    M = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(G, N))
    ids = _labels(41, N, C)
    P, LFC, labels = gficf_amd.cluster_markers(M, ids)
    ref = mk.markers_sparse(M, ids, C)
    R = M.tocsr()
    n1 = np.bincount(ids, minlength=C)
    for g in range(G):
        row = R[g]
        cl = ids[row.indices]
        for c in range(C):
            s1, s2 = math.fsum(row.data[cl == c]), math.fsum(row.data[cl != c])
            n2 = N - n1[c]
            with np.errstate(invalid="ignore"):
                ref["lfc"][g, c] = np.log2(((s1 + n1[c]) / n1[c]) / ((s2 + n2) / n2))
    _check_range(P, LFC, labels, ref)
