"""GPU: libgficf_svds.so, the exact truncated SVD behind randomized="svds" (include/gficf_svds.h).

The yardstick is LAPACK on the densified (and, for the centred case, centred) matrix.  The tolerance is the project's rule
(tests/helpers/rsvd_np.tolerance): a figure of the device against LAPACK may be 32 x the same figure of the f64 numpy port of
the method (tests/helpers/svds_np.py) against LAPACK, never below 64 eps.  The figures are those of rsvd_np.deviations — d
relative to d[0], sign-aligned cells / d[0], genes — with one change: components whose values coincide or nearly coincide
(closer than 1e-6 d[0]) are compared as a group, by the projector of their span, since LAPACK's choice within the group is
arbitrary; zero components (rank below k) are asserted to be exactly zero instead.  Every figure is printed before it is
asserted."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import gficf_amd
from gficf_amd import GficfError
from tests.helpers import rsvd_np as rp
from tests.helpers import svds_np as sn
from tests.helpers.svds_cases import _device_form, _figures, _groups, _start, check_direct_residual, check_properties

pytestmark = pytest.mark.gpu

EPS = rp.EPS
TOL = 1e-10
SEED = 5


def _sparse(nrows, ncols, density, seed, empty_every=7, zero_every=11):
    """CSC with empty columns, empty rows and explicitly stored zeros (the shape of tests/test_pca_gpu.py's _sparse)."""
    rng = np.random.default_rng(seed)
    A = sp.random(nrows, ncols, density=density, format="csc", random_state=rng, data_rvs=rng.standard_normal)
    D = A.toarray() * (np.arange(ncols) % empty_every != 3)
    D[np.arange(nrows) % 13 == 5, :] = 0.0
    A = sp.csc_matrix(D)
    A.sort_indices()
    A.data[::zero_every] = 0.0
    assert (np.diff(A.indptr) == 0).any() and (A.data == 0).any()
    return A


def _twice():
    B = sp.random(21, 37, 0.4, random_state=np.random.default_rng(SEED), data_rvs=np.random.default_rng(SEED + 2).standard_normal)
    return sp.csc_matrix(sp.block_diag([B, B]))


# name -> (genes x cells matrix, k, b, m, centre)
CASES = {
    "restart_m40": lambda: (rp.planted_sparse(600, 320, 12, SEED), 10, 8, 40, False),
    "restart_m32": lambda: (rp.planted_sparse(600, 320, 12, SEED), 10, 8, 32, False),
    "transposed": lambda: (rp.planted_sparse(200, 640, 12, SEED), 10, 8, 40, False),
    "single_cycle": lambda: (rp.planted_sparse(300, 80, 6, SEED), 6, 8, 80, False),
    "k1": lambda: (rp.planted_sparse(300, 80, 6, SEED), 1, 8, 24, False),
    "full_83": lambda: (sp.csc_matrix(sp.random(83, 301, 0.2, random_state=np.random.default_rng(SEED))), 83, 8, 83, False),
    "flat": lambda: (sn.flat(SEED), 10, 8, 40, False),
    "twice": lambda: (_twice(), 6, 8, 24, False),
    "centred": lambda: (rp.planted_sparse(600, 320, 12, SEED), 10, 8, 40, True),
    "segments": lambda: (sp.csc_matrix(sp.random(12, 3000, 0.9, random_state=np.random.default_rng(SEED))), 12, 8, 12, False),
    "rank_3": lambda: (rp.blocks(120, 60, [40, 30, 20], [10, 8, 6], [3.0, 2.0, 1.0])[0], 5, 8, 60, False),
    "empty": lambda: (_sparse(150, 400, 0.08, SEED), 8, 8, 40, False),
}
_cache: dict = {}


def _case(name):
    """(M, k, m, centre, start, LAPACK, port, device), computed once."""
    if name not in _cache:
        M, k, b, m, centre = CASES[name]()
        start = _start(min(M.shape), b)
        want = sn.dense_svd(M, k, centre)
        port = sn.svds(M, start, k, m, tol=TOL, centre=centre)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got = gficf_amd.svds(M, k, centre=centre, tol=TOL, m=m, start=start)
        got["genes"] = got["v"]
        for r in (want, port, got):
            for v in r.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        _cache[name] = (M, k, m, centre, start, want, port, got)
    return _cache[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_matches_lapack_within_the_ports_own_deviation(name):
    M, k, m, centre, start, want, port, got = _case(name)
    fp, fg = _figures(want, port), _figures(want, got)
    print(name, "port", fp, "device", fg, "ratio", {q: fg[q] / max(fp[q], EPS) for q in fp},
          "cycles", got["cycles"], port["cycles"], "products", got["products"], port["products"])
    for q in fp:
        assert fg[q] <= rp.tolerance(fp[q]), (name, q, fg[q], fp[q])
    assert got["cells"].shape == (M.shape[1], k) and got["genes"].shape == (M.shape[0], k)
    assert got["converged"] == k or got["exhausted"]
    if centre:
        assert np.allclose(got["centre"], M.toarray().mean(axis=1), rtol=1e-13, atol=0)
    else:
        assert got["centre"] is None


@pytest.mark.parametrize("name", sorted(CASES))
def test_properties_orthonormal_genes_cells_sign_rule_order(name):
    M, k, m, centre, start, want, port, got = _case(name)
    check_properties(name, M, centre, k, port, got)


@pytest.mark.parametrize("name", sorted(CASES))
def test_direct_residual_on_the_host(name):
    M, k, m, centre, start, want, port, got = _case(name)
    check_direct_residual(name, M, centre, port, got)


def test_flat_spectrum_converges_where_the_sketch_is_percent_level_off():
    M, k, m, centre, start, want, port, got = _case("flat")
    tau = rp.tau(max(M.shape))
    assert got["converged"] == 10 and not got["exhausted"] and got["cycles"] > 1
    assert (got["residuals"] <= np.maximum(TOL, tau * got["d"][0] ** 2 / got["d"] ** 2)).all(), got["residuals"]
    sk = gficf_amd.rsvd(M, k)
    off = np.abs(sk["d"] - want["d"]).max() / want["d"][0]
    print("rsvd off", off, "svds off", np.abs(got["d"] - want["d"]).max() / want["d"][0])
    assert off > 1e-3
    # the same through the mirror: on the code before randomized="svds" existed the string was truthy and ran the sketch
    data = gficf_amd.runPCA({"gficf": M}, dim=k, randomized="svds")
    d = np.linalg.norm(data["pca"]["cells"], axis=0)
    dp = sn.svds(M, np.random.default_rng(180582).standard_normal((min(M.shape), 8)), k, tol=TOL)["d"]
    assert np.abs(d - want["d"]).max() / want["d"][0] <= rp.tolerance(np.abs(dp - want["d"]).max() / want["d"][0])
    assert data["pca"]["svds"]["converged"] == k


def test_every_value_twice_gives_the_planes():
    M, k, m, centre, start, want, port, got = _case("twice")
    assert np.abs(want["d"][0::2] - want["d"][1::2]).max() < 1e-12 * want["d"][0]
    assert [len(g) for g in _groups(want["d"], 1e-6 * want["d"][0])] == [2, 2, 2]
    assert got["converged"] == 6 and got["cycles"] > 5


def test_rank_below_k_gives_exact_zeros():
    M, k, m, centre, start, want, port, got = _case("rank_3")
    _, d, U, V = rp.blocks(120, 60, [40, 30, 20], [10, 8, 6], [3.0, 2.0, 1.0])
    devp = np.abs(port["d"][:3] - d).max() / d[0]
    assert np.abs(got["d"][:3] - d).max() / d[0] <= rp.tolerance(devp)
    assert (got["d"][3:] == 0).all() and (got["genes"][:, 3:] == 0).all() and (got["cells"][:, 3:] == 0).all() and got["exhausted"]
    assert np.abs(got["genes"][:, :3] - V).max() <= rp.tolerance(np.abs(port["genes"][:, :3] - V).max())


@pytest.mark.parametrize("name", ["restart_m40", "transposed", "centred"])
def test_same_bits_twice_on_the_device_form_and_with_a_drawn_start(name):
    M, k, m, centre, start, want, port, got = _case(name)
    again = gficf_amd.svds(M, k, centre=centre, tol=TOL, m=m, start=start)
    for q in ("d", "cells", "v", "residuals"):
        assert np.array_equal(again[q], got[q]), q
    dev = _device_form(M, k, 8, m, centre, start)
    assert np.array_equal(dev["d"], got["d"]) and np.array_equal(dev["cells"], got["cells"]) and np.array_equal(dev["genes"], got["genes"])
    assert np.array_equal(dev["residuals"], got["residuals"])
    assert list(dev["info"]) == [got["cycles"], got["products"], got["converged"], int(got["exhausted"])]
    if centre:
        assert np.array_equal(dev["centre"], got["centre"])
    drawn = gficf_amd.svds(M, k, centre=centre, tol=TOL, m=m, seed=77)
    given = gficf_amd.svds(M, k, centre=centre, tol=TOL, m=m, start=np.random.default_rng(77).standard_normal((min(M.shape), 8)))
    assert np.array_equal(drawn["d"], given["d"]) and np.array_equal(drawn["cells"], given["cells"])


def test_one_cycle_is_reported_not_hidden():
    M, k, m, centre, start, want, port, got = _case("flat")
    with pytest.warns(UserWarning, match=r"only \d+ of the 10 singular values converged"):
        r = gficf_amd.svds(M, k, tol=TOL, m=m, start=start, max_cycles=1)
    assert r["converged"] < 10 and r["cycles"] == 1 and not r["exhausted"]
    assert np.isfinite(r["d"]).all() and np.isfinite(r["cells"]).all() and np.isfinite(r["v"]).all() and np.isfinite(r["residuals"]).all()
    assert (r["residuals"] > TOL).sum() >= 10 - r["converged"] and r["residuals"].max() > 1e-3
    p1 = sn.svds(M, start, k, m, tol=TOL, max_cycles=1)
    assert p1["converged"] == r["converged"] and np.allclose(p1["residuals"], r["residuals"], rtol=1e-6, atol=1e-14)


def _raises(status, fn):
    with pytest.raises(GficfError) as e:
        fn()
    assert e.value.status == status, (e.value.status, str(e.value))


def test_error_codes_and_the_context_stays_usable():
    M, k, m, centre, start, want, port, got = _case("restart_m40")
    n = min(M.shape)
    _raises("GFICF_ERR_INVALID_ARG", lambda: gficf_amd.svds(M, 0, m=40))
    _raises("GFICF_ERR_INVALID_ARG", lambda: gficf_amd.svds(M, 10, m=25))                          # m < k + 2 b with m < n
    _raises("GFICF_ERR_INVALID_ARG", lambda: gficf_amd.svds(M, 10, start=_start(n, 33)))
    _raises("GFICF_ERR_INVALID_ARG", lambda: gficf_amd.svds(M, 10, m=129))
    bad = M.copy(); bad.data[17] = np.nan
    _raises("GFICF_ERR_BAD_VALUE", lambda: gficf_amd.svds(bad, k, m=m, start=start))
    st = start.copy(); st[3, 2] = np.nan
    _raises("GFICF_ERR_BAD_VALUE", lambda: gficf_amd.svds(M, k, m=m, start=st))
    _raises("GFICF_ERR_CAPACITY", lambda: _device_form(M, k, 8, m, False, start, ws_cut=4096))
    ip = M.indptr.copy(); ip[10] = ip[9] - 1                                                       # not monotone, on the device
    _raises("GFICF_ERR_BAD_CSC", lambda: _device_form(M, k, 8, m, False, start, colptr=ip))
    r = gficf_amd.svds(M, k, tol=TOL, m=m, start=start)
    assert np.array_equal(r["d"], got["d"])


# ------------------------------------------------------------------------------------------------ the mirror, end to end
@pytest.fixture(scope="module")
def e2e():
    M, group = rp.planted_counts(N=700, C=5, G=600, seed=31)
    return gficf_amd.gficf(M, verbose=False)


def test_runpca_runlsa_computepcadim_with_svds(e2e):
    M = e2e["gficf"]
    n = min(M.shape)
    start = np.random.default_rng(180582).standard_normal((n, 8))
    for fn, centre in ((gficf_amd.runPCA, True), (gficf_amd.runPCA, False), (gficf_amd.runLSA, False)):
        data = fn(dict(e2e), dim=10, centre=centre, randomized="svds")
        want = sn.dense_svd(M, 10, centre)
        port = sn.svds(M, start, 10, tol=TOL, centre=centre)
        d = np.linalg.norm(data["pca"]["cells"], axis=0)
        got = {"d": d, "cells": data["pca"]["cells"], "genes": data["pca"]["genes"]}
        fp, fg = _figures(want, port), _figures(want, got)
        print(fn.__name__, centre, "port", fp, "device", fg)
        for q in fp:
            assert fg[q] <= rp.tolerance(fp[q]), (q, fg[q], fp[q])
        assert sorted(data["pca"]["svds"]) == ["converged", "cycles", "residuals"] and data["pca"]["svds"]["converged"] == 10
        assert data["dimPCA"] == 10 and data["pca"]["centre"] is centre
        proj = gficf_amd.pca_project(data, M)
        # two f64 evaluations of the same G-term inner products: each within G eps sum |a||v| <= G eps d[0] of the exact value
        assert M.shape[0] <= M.shape[1] and np.abs(proj - data["pca"]["cells"]).max() / d[0] <= 2 * M.shape[0] * EPS
    assert "svds" not in gficf_amd.runPCA(dict(e2e), dim=10)["pca"]
    data = gficf_amd.clustcells(data, k=15, verbose=False)
    assert len(data["cluster"]) == M.shape[1]
    # computePCADim: the elbow rule on the exact values
    w50 = sn.dense_svd(M, 50)["d"]
    rule = gficf_amd.pca_dim_rule(w50)
    if rule is None:
        with pytest.raises(ValueError, match="elbow rule"):
            gficf_amd.computePCADim(dict(e2e), randomized="svds")
    else:
        assert gficf_amd.computePCADim(dict(e2e), randomized="svds")["dimPCA"] == rule
    r50 = gficf_amd.svds(M, 50)
    p50 = sn.svds(M, start, 50, tol=TOL)
    assert np.abs(r50["d"] - w50).max() / w50[0] <= rp.tolerance(np.abs(p50["d"] - w50).max() / w50[0])
