"""libgficf_tmm.so on the GPU against its NumPy oracle (tests/helpers/tmm_np.py, canonical keys) and against answers derived by
hand: the trim decisions (n, kept), the reference column and the order statistics exactly, the sums to the rounding of their
order, cpm bit for bit; both rank paths; the Python mirror."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import gficf_amd
from gficf_amd import GficfError, _tmm_lib, synth
from tests.helpers import tmm_np

pytestmark = pytest.mark.gpu

# The sums differ from NumPy's by their order only, log2 and exp2 by their last bit.  Largest relative differences measured on the
# MI355X over the inputs of this file: norm.factors 1.75e-15 and factors.raw 1.08e-15 (counts_csc(2000, 300, 0.07) and the edge
# cases), sq 1.46e-14 (the columns of 8 232 entries), f75 and lib.size 0 (integer counts: exact sums, the same operations in
# the same order).  Each bound is eight times its figure, and none is above 1e-12.
REL = {"norm.factors": 8 * 1.75e-15, "factors.raw": 8 * 1.08e-15, "sq": 8 * 1.46e-14, "f75": 0.0, "lib.size": 0.0}
assert max(REL.values()) <= 1e-12


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(a - b) / np.abs(b)
    return float(np.nanmax(np.where(a == b, 0.0, d))) if a.size else 0.0


def compare(got, want, what, integer=True):
    """The exact parts exactly; the rest printed, then held to REL."""
    assert got["refColumn"] == want["refColumn"] and got["Gprime"] == want["Gprime"]
    assert np.array_equal(got["n"], want["n"]) and np.array_equal(got["kept"], want["kept"])
    assert np.array_equal(got["ostat"], want["ostat"])
    if integer:
        assert np.array_equal(got["lib.size"], want["lib.size"])
    fig = {k: rel(got[k], want[k]) for k in ("norm.factors", "factors.raw", "f75", "sq", "lib.size")}
    print(what, {k: f"{v:.3g}" for k, v in fig.items()})
    assert all(fig[k] <= REL[k] for k in fig), fig
    assert abs(np.log(got["norm.factors"]).mean()) < 1e-14


def same_bits(a, b):
    for k in ("norm.factors", "factors.raw", "lib.size", "f75", "sq", "ostat", "n", "kept"):
        assert np.array_equal(a[k], b[k]), k
    assert a["refColumn"] == b["refColumn"] and a["Gprime"] == b["Gprime"]


@functools.lru_cache(maxsize=None)
def counts():
    colptr, rowidx, x = synth.counts_csc(2000, 300, 0.07)
    M = sp.csc_matrix((x, rowidx, colptr), shape=(2000, 300))
    return M, M.toarray()


@functools.lru_cache(maxsize=None)
def edge():
    X, M = tmm_np.edge_matrix()
    return M, X, tmm_np.calc_norm_factors(X)


def test_sparse_counts_take_the_sq_branch():
    M, X = counts()
    want = tmm_np.calc_norm_factors(X)
    assert np.median(want["f75"]) < 1e-20
    got = gficf_amd.calcNormFactors(M)
    assert set(got) >= {"norm.factors", "lib.size", "refColumn", "f75", "n", "kept"}
    compare(got, want, "counts_csc(2000, 300, 0.07)")
    assert (got["kept"] < got["n"]).any() and got["n"][got["refColumn"]] == (X[:, got["refColumn"]] > 0).sum()
    same_bits(got, gficf_amd.calcNormFactors(M))                         # the same call twice


def test_dense_counts_take_the_f75_branch():
    X = tmm_np.gamma_poisson()
    want = tmm_np.calc_norm_factors(X)
    assert np.median(want["f75"]) > 1e-20 and (want["ostat"][0] > 0).any()
    compare(gficf_amd.calcNormFactors(sp.csc_matrix(X)), want, "gamma_poisson(3000, 200)")


def test_trim_boundaries_and_degenerate_cells():
    M, X, want = edge()
    assert M.nnz == (X > 0).sum() + 1 and want["Gprime"] < 780           # a stored zero; all-zero rows
    got = gficf_amd.calcNormFactors(M)
    compare(got, want, "edge cases")
    k = len(tmm_np.EDGE_N)
    assert list(got["n"][1:k + 1]) == list(tmm_np.EDGE_N) and got["refColumn"] == 0
    assert got["factors.raw"][0] == 1 and got["factors.raw"][k + 1] == 1   # the reference and its copy: every logR is 0
    assert got["factors.raw"][1] == 1 and got["kept"][1] == 0             # n = 0
    assert got["n"][k + 2] == 1 and got["lib.size"][k + 3] == 0 and got["f75"][k + 3] == 0 and got["factors.raw"][k + 3] == 1
    assert np.isfinite(got["norm.factors"]).all()


def test_reference_given_and_plain_mean():
    M, X, _ = edge()
    k = len(tmm_np.EDGE_N)
    compare(gficf_amd.calcNormFactors(M, refColumn=k), tmm_np.calc_norm_factors(X, refColumn=k), "refColumn given")
    compare(gficf_amd.calcNormFactors(M, doWeighting=False), tmm_np.calc_norm_factors(X, doWeighting=False), "doWeighting=False")
    compare(gficf_amd.calcNormFactors(M, logratioTrim=.1, sumTrim=.2), tmm_np.calc_norm_factors(X, logratioTrim=.1, sumTrim=.2), "other trims")
    # a single-gene cell against a single-gene reference: v = 0, logR = 0, 0 / 0 -> 1
    S = sp.csc_matrix(np.array([[0.0, 0, 2], [3, 7, 1], [0, 0, 4]]))
    got = gficf_amd.calcNormFactors(S, refColumn=0)
    compare(got, tmm_np.calc_norm_factors(S.toarray(), refColumn=0), "single genes")
    assert list(got["n"]) == [1, 1, 1] and list(got["factors.raw"][:2]) == [1, 1]


def test_int32_and_int64_colptr_give_the_same_bits():
    M, _, _ = edge()
    a, b = M.copy(), M.copy()
    a.indptr, b.indptr = M.indptr.astype(np.int32), M.indptr.astype(np.int64)
    same_bits(gficf_amd.calcNormFactors(a), gficf_amd.calcNormFactors(b))
    assert np.array_equal(gficf_amd.cpm(a).data, gficf_amd.cpm(b).data)


def test_bad_values_are_errors_and_the_context_stays_usable():
    M, _, want = edge()
    for bad in (-1.0, np.nan, np.inf):
        B = M.copy()
        B.data = B.data.copy()
        B.data[5] = bad
        with pytest.raises(GficfError, match="negative, NaN or infinite"):
            gficf_amd.calcNormFactors(B)
        with pytest.raises(GficfError, match="negative, NaN or infinite"):
            gficf_amd.cpm(B)
    B = M.copy()
    B.indices = B.indices.copy()
    B.indices[-1] = 800
    with pytest.raises(GficfError, match="row index outside"):
        gficf_amd.calcNormFactors(B)
    got = gficf_amd.calcNormFactors(M)
    assert np.array_equal(got["n"], want["n"]) and np.array_equal(got["kept"], want["kept"])


def test_both_rank_paths_give_the_same_bits():
    M, X, want = edge()
    small = gficf_amd.calcNormFactors(M, max_lds_n=64)                    # n = 65 and 500, the reference and its copy: the counting kernel
    assert (want["n"] > 64).sum() >= 4 and (want["n"] == 64).any() and (want["n"] == 63).any()
    same_bits(small, gficf_amd.calcNormFactors(M))
    compare(small, want, "max_lds_n = 64")
    dense = sp.csc_matrix(tmm_np.gamma_poisson(600, 20, seed=8))           # the quantile selected by counting, not from the sorted list
    same_bits(gficf_amd.calcNormFactors(dense, max_lds_n=64), gficf_amd.calcNormFactors(dense))
    with pytest.raises(GficfError, match="max_lds_n"):
        gficf_amd.calcNormFactors(M, max_lds_n=_tmm_lib.LDS_N + 1)


def test_cells_between_the_two_lds_tiers():
    # n between the first tier's 2 048 keys and the capacity: ranked by the second launch of the LDS kernel; with the capacity
    # lowered to 2 048 the same cells go to the counting kernel instead
    rng = np.random.default_rng(17)
    X = rng.poisson(rng.lognormal(1.0, 1.0, 3000)[:, None] * np.array([1.0, 1.4, .8, 2.0, .05, 1.1])[None, :]).astype(np.float64)
    want = tmm_np.calc_norm_factors(X)
    assert (want["n"] > 2048).sum() >= 4 and (want["n"] < 2048).any() and 2 * 8 * 2048 < 64 * 1024
    got = gficf_amd.calcNormFactors(sp.csc_matrix(X))
    compare(got, want, "6 columns of 3 000 genes")
    same_bits(got, gficf_amd.calcNormFactors(sp.csc_matrix(X), max_lds_n=2048))


def test_bulk_like_columns_longer_than_the_lds_lists():
    rng = np.random.default_rng(21)
    G = _tmm_lib.LDS_N + 40
    X = 1.0 + rng.poisson(rng.lognormal(1.0, 1.0, G)[:, None] * np.array([1.0, 1.5, .7, 2.2])[None, :])
    want = tmm_np.calc_norm_factors(X)
    assert (want["n"] == G).all()
    compare(gficf_amd.calcNormFactors(sp.csc_matrix(X)), want, "4 dense columns")


def test_cpm_is_bit_for_bit():
    M, X = counts()
    res = gficf_amd.calcNormFactors(M)
    got = gficf_amd.cpm(M, res["lib.size"], res["norm.factors"])
    assert np.array_equal(got.indptr, M.indptr) and np.array_equal(got.indices, M.indices)
    want = tmm_np.cpm(X, res["lib.size"], res["norm.factors"])
    assert np.array_equal(got.toarray(), np.where(X > 0, want, 0.0))
    assert np.array_equal(gficf_amd.cpm(M, norm_factors=res["norm.factors"]).data, got.data)     # lib.size = colSums
    assert np.array_equal(gficf_amd.cpm(M).toarray(), np.where(X > 0, X / (1e-6 * (X.sum(axis=0) * 1.0))[None, :], 0.0))
    Me, _, _ = edge()                                                     # an empty column, a stored zero
    e = gficf_amd.cpm(Me)
    assert e.nnz == Me.nnz and np.isfinite(e.data).all()


def test_derived_answers_hold_on_the_device():
    X = tmm_np.multiples_matrix()
    M = sp.csc_matrix(X)
    res = gficf_amd.calcNormFactors(M, refColumn=0)
    tmm_np.check_multiples(X, res, gficf_amd.cpm(M, res["lib.size"], res["norm.factors"]).toarray())
    X, changed = tmm_np.boosted_matrix()
    M = sp.csc_matrix(X)
    res = gficf_amd.calcNormFactors(M, refColumn=0)
    tmm_np.check_boosted(X, changed, res, gficf_amd.cpm(M, res["lib.size"], res["norm.factors"]).toarray())


def test_device_resident_entries_give_the_host_entrys_bits():
    import torch

    M, _, _ = edge()
    G, N = M.shape
    host = gficf_amd.calcNormFactors(M)
    ops = gficf_amd.HipOps(0)
    dev = torch.device("cuda", 0)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    colptr, rowidx, x = t(M.indptr.astype(np.int64)), t(M.indices.astype(np.int32)), t(M.data)
    nz = np.diff(M.indptr)
    big = nz > 64
    ws = torch.empty(ops.tmm_workspace_bytes(G, N, int(big.sum()), int(nz[big].sum())), dtype=torch.uint8, device=dev)
    lib, sq, f75, fac = (torch.empty(N, dtype=torch.float64, device=dev) for _ in range(4))
    ostat = torch.empty((2, N), dtype=torch.float64, device=dev)
    gp, n, kept = torch.empty(1, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    ops.tmm_stats(G, N, colptr, rowidx, x, int(nz.max()), ws, lib, sq, f75, ostat, gp, max_lds_n=64)
    ops.tmm_factors(G, N, colptr, rowidx, x, int(nz.max()), host["refColumn"], lib, ws, fac, n, kept, max_lds_n=64, big_cells=int(big.sum()),
                    big_entries=int(nz[big].sum()), fresh=False)
    out = torch.empty_like(x)
    ops.tmm_cpm(N, colptr, x, lib, t(host["norm.factors"]), ws, out)
    ops.tmm_sync(ws)
    for k, v in (("lib.size", lib), ("sq", sq), ("f75", f75), ("ostat", ostat), ("factors.raw", fac), ("n", n), ("kept", kept)):
        assert np.array_equal(v.cpu().numpy(), host[k]), k
    assert int(gp.item()) == host["Gprime"]
    assert np.array_equal(out.cpu().numpy(), gficf_amd.cpm(M, host["lib.size"], host["norm.factors"]).data)
    # fewer big cells announced than there are: a deferred error, not a wild write
    ops.tmm_factors(G, N, colptr, rowidx, x, int(nz.max()), host["refColumn"], lib, ws, fac, n, kept, max_lds_n=64, big_cells=1, big_entries=int(nz[big].sum()))
    with pytest.raises(GficfError, match="beyond the LDS capacity"):
        ops.tmm_sync(ws)


# ------------------------------------------------------------------ the mirror
@functools.lru_cache(maxsize=None)
def clustered():
    _, X = counts()
    X = X.copy()
    X[:60, :100] += np.random.default_rng(1).poisson(3.0, (60, 100))      # markers of the first cluster
    return sp.csc_matrix(X), np.repeat(["a", "b", "c"], 100)


def test_gficf_with_tmm_keeps_gficf_and_stores_cpms():
    M, _ = clustered()
    plain = gficf_amd.gficf(M, normalize=False, verbose=False)
    data = gficf_amd.gficf(M, normalize="tmm", verbose=False)
    assert data["param"]["normalized"] is True and plain["param"]["normalized"] is False
    for k in ("data", "indices", "indptr"):
        assert np.array_equal(getattr(data["gficf"], k), getattr(plain["gficf"], k)), k
    assert np.array_equal(data["genes"], plain["genes"]) and np.array_equal(data["w"], plain["w"])
    res = gficf_amd.calcNormFactors(plain["rawCounts"])
    want = gficf_amd.cpm(plain["rawCounts"], res["lib.size"], res["norm.factors"])
    assert np.array_equal(data["rawCounts"].data, want.data) and np.array_equal(data["rawCounts"].indices, want.indices)
    assert np.array_equal(gficf_amd.normCounts(M, 1, .05, True, verbose=False).toarray(), want.toarray())
    assert gficf_amd.normCounts(M, 1, .05, False).shape == want.shape
    with pytest.warns(UserWarning, match='normalize="tmm"'):
        warned = gficf_amd.gficf(M, normalize=True, verbose=True)
    assert np.array_equal(warned["rawCounts"].data, plain["rawCounts"].data) and warned["param"]["normalized"] is True


def test_find_cluster_markers_with_tmm():
    M, labels = clustered()
    data = gficf_amd.gficf(M, normalize=False, verbose=False)
    data["community"] = data["cluster"] = labels
    a = gficf_amd.findClusterMarkers(dict(data), hvg=False, cpms="tmm", verbose=False)["de.genes"]
    b = gficf_amd.findClusterMarkers(dict(data), hvg=False, cpms=gficf_amd.normCounts(data["rawCounts"], 2, 0, True, verbose=False), verbose=False)["de.genes"]
    assert len(a) > 0 and a.equals(b) and (a["cluster"] == "a").any()
    with pytest.warns(UserWarning, match='raw counts.*cpms="tmm"'):
        c = gficf_amd.findClusterMarkers(dict(data), hvg=False, verbose=False)["de.genes"]
    assert not a.equals(c)
    done = gficf_amd.gficf(M, normalize="tmm", verbose=False)             # already normalised: normCounts(rawCounts, 2, 0, FALSE)
    done["community"] = done["cluster"] = labels
    d = gficf_amd.findClusterMarkers(dict(done), hvg=False, cpms="tmm", verbose=False)["de.genes"]
    assert d.equals(gficf_amd.findClusterMarkers(dict(done), hvg=False, cpms=done["rawCounts"], verbose=False)["de.genes"]) and d.equals(a)
