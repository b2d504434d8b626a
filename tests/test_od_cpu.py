"""No GPU: the oracle of libgficf_od.so (tests/helpers/od_np.py, the yardstick of tests/test_od_gpu.py) against independent
things (SciPy's natural cubic spline, its F and chi-square distributions, p.adjust), the planted fixture's margins, the header
against its loader and the Makefile, and the argument handling of the Python mirror."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.interpolate
import scipy.sparse as sp
import scipy.stats

import gficf_amd
from tests.helpers import od_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_loader_name_the_same_entries():
    from gficf_amd import _od_lib

    text = open(os.path.join(ROOT, "include", "gficf_od.h")).read()
    body = text[text.index("extern \"C\""):]
    declared = re.findall(r"\b(gficf_od_\w+)\s*\(([^;]*)\)\s*;", body)
    assert set(n for n, _ in declared) == set(_od_lib.SIGNATURES) and len(declared) == 12
    for name, args in declared:
        n = 0 if args.strip() == "void" else args.count(",") + 1
        assert n == len(_od_lib.SIGNATURES[name][1]), name
    assert "#define GFICF_OD_ABI_VERSION 1" in text and _od_lib.ABI_VERSION == 1
    assert re.search(rf"#define\s+GFICF_OD_K_MAX\s+{_od_lib.K_MAX}\b", text) and re.search(rf"#define\s+GFICF_OD_INFO\s+{len(_od_lib.INFO)}\b", text)
    assert "has NOT been measured" in text                                       # how far the cr fit is from mgcv's default basis
    core = open(os.path.join(ROOT, "include", "gficf_hip.h")).read()
    assert re.search(r"#define\s+GFICF_HIP_ABI_VERSION\s+7\b", core)
    assert "#define GFICF_HVG_ABI_VERSION 1" in open(os.path.join(ROOT, "include", "gficf_hvg.h")).read()


def test_makefile_builds_the_library_with_the_others():
    csrc = os.path.join(ROOT, "gficf_amd", "csrc")
    build = subprocess.run(["make", "-n", "-B", "-C", csrc, "all"], capture_output=True, text=True, check=True).stdout.splitlines()
    link = [ln for ln in build if " -o ../libgficf_od.so " in ln]
    assert len(link) == 1 and re.search(r"hipcc --offload-arch=gfx950 -shared -fPIC -o \.\./libgficf_od\.so od\.o -L\.\. -lgficf_hip -lgficf_hvg\b", link[0])
    comp = [ln for ln in build if ln.endswith(" -o od.o")]
    assert len(comp) == 1 and "-ffp-contract=off" in comp[0] and "--offload-arch=gfx950" in comp[0] and "fast-math" not in comp[0]
    assert build.index(link[0]) > max(i for i, ln in enumerate(build) if " -o ../libgficf_hvg.so " in ln or ln.endswith(" -o od.o"))
    clean = subprocess.run(["make", "-n", "-C", csrc, "clean"], capture_output=True, text=True, check=True).stdout
    assert re.search(r"^rm -f .*\bod\.o\b.* \.\./libgficf_od\.so\b", clean, re.M)


def test_loader(monkeypatch):
    from gficf_amd import _od_lib

    L = _od_lib.load()
    assert isinstance(L, ctypes.CDLL) and _od_lib.load() is L and L.gficf_od_abi_version() == _od_lib.ABI_VERSION
    for sym, (res, args) in _od_lib.SIGNATURES.items():
        fn = getattr(L, sym)
        assert fn.restype is res and list(fn.argtypes) == list(args), sym
    lists = L.gficf_od_workspace_bytes(23000, 0)
    assert 50 * 23000 < lists < 200 * 23000 + (1 << 20)
    assert L.gficf_od_workspace_bytes(23000, 54000) >= lists + 8 * 54000 - 256
    assert L.gficf_od_workspace_bytes(0, 0) == 0 and L.gficf_od_workspace_bytes(10, -1) == 0
    monkeypatch.setattr(_od_lib, "LIB_PATH", os.path.join(os.path.dirname(_od_lib.LIB_PATH), "libgficf_od_missing.so"))
    with pytest.raises(ImportError, match="not found: build it with"):
        _od_lib.load()


# ------------------------------------------------------------------ the oracle's spline against what defines it
KNOTS = np.array([0.3, 1.1, 1.7, 3.2, 5.9])


def test_design_row_times_knot_values_is_scipys_natural_cubic_spline():
    rng = np.random.default_rng(0)
    F, S = od_np.basis(KNOTS)
    x = np.concatenate([rng.uniform(KNOTS[0], KNOTS[-1], 200), KNOTS])
    X = od_np.design(KNOTS, F, x)
    np.testing.assert_allclose(X.sum(axis=1), 1.0, rtol=0, atol=1e-13)             # the rows sum to 1
    for _ in range(3):
        vals = rng.normal(size=5)
        want = scipy.interpolate.CubicSpline(KNOTS, vals, bc_type="natural")(x)
        np.testing.assert_allclose(X @ vals, want, rtol=1e-12, atol=1e-12)
    # the penalty annihilates constants and straight lines and is the integral of the squared second derivative
    assert np.abs(S @ np.ones(5)).max() < 1e-13 and np.abs(S @ KNOTS).max() < 1e-13
    vals = rng.normal(size=5)
    cs = scipy.interpolate.CubicSpline(KNOTS, vals, bc_type="natural")
    g = np.linspace(KNOTS[0], KNOTS[-1], 200001)
    np.testing.assert_allclose(vals @ S @ vals, np.trapezoid(cs(g, 2) ** 2, g), rtol=1e-6)


def test_knots_are_place_knots():
    x = np.array([5.0, 1.0, 1.0, 2.0, 9.0, 4.0, 4.0, 7.0])                          # distinct: 1 2 4 5 7 9
    np.testing.assert_allclose(od_np.place_knots(x, 5), [1.0, 2.5, 4.5, 6.5, 9.0])  # t = 0, 1.25, 2.5, 3.75, 5
    assert od_np.place_knots(x, 7) is None
    np.testing.assert_array_equal(od_np.place_knots(x, 6), [1, 2, 4, 5, 7, 9])


def test_the_limits_of_the_smoothing_parameter():
    rng = np.random.default_rng(1)
    m = rng.uniform(0.3, 5.9, 60)
    v = np.sin(m) + rng.normal(0, 0.1, 60)
    kn = od_np.place_knots(m, 5)
    F, S = od_np.basis(kn)
    X = od_np.design(kn, F, m)
    line = np.polyval(np.polyfit(m, v, 1), m)
    np.testing.assert_allclose(od_np.penalised_fit(X, S, v, 1e10), line, atol=1e-6)    # sp -> infinity: the least-squares line
    # sp = 0 and k = n distinct points: the fit interpolates
    m5, v5 = np.sort(rng.uniform(0, 4, 5)), rng.normal(size=5)
    F5, S5 = od_np.basis(m5)
    np.testing.assert_allclose(od_np.penalised_fit(od_np.design(m5, F5, m5), S5, v5, 0.0), v5, atol=1e-12)
    # the spectral GCV of the contract is the GCV of the influence matrix, and the fixed search finds a minimum of it
    spec = od_np.spectrum(X, S, v)
    for lam in (1e-6, 1e-2, 1.0, 1e3):
        np.testing.assert_allclose(od_np.gcv_spectral(spec, lam), od_np.gcv_dense(X, S, v, lam), rtol=1e-8)
    lam = od_np.search_lambda(spec)
    g0 = od_np.gcv_spectral(spec, lam)[0]
    assert all(g0 <= od_np.gcv_spectral(spec, math.exp(r))[0] * (1 + 1e-12) for r in od_np.RHO_GRID)
    assert g0 <= min(od_np.gcv_spectral(spec, lam * f)[0] for f in (0.9, 1.1)) * (1 + 1e-12)


def test_the_line_is_taken_below_one_and_a_half_k_valid_genes_and_below_k_distinct_weights():
    for G, want in ((1, 1), (6, 2), (7, 2), (8, 5)):                                # n < 1.5 * 5 = 7.5
        m, var, nobs = np.linspace(1, 2, G), np.exp(np.linspace(0, 1, G) ** 2), np.full(G, 5)
        r = od_np.fit(m, var, nobs)
        assert r["basis"] == want, G
        if 1 < G < 8:
            np.testing.assert_allclose(r["fit"], np.polyval(np.polyfit(m, np.log(var), 1), m), atol=1e-12)
    m, var, nobs, _ = od_np.moments_case(40, ties=4)
    assert od_np.fit(m, var, nobs)["basis"] == 2 and len(np.unique(m)) == 4
    m, var, nobs, _ = od_np.moments_case(40, ties=5)
    r = od_np.fit(m, var, nobs)
    assert r["basis"] == 5 and np.array_equal(r["knots"], np.unique(m[r["valid"]]))


# ------------------------------------------------------------------ the special functions
def test_log_pf_is_scipys_f_distribution_where_that_is_finite():
    a = np.array([0.5, 1, 2.5, 50, 1e3])
    res = np.array([-40, -3, -1e-9, 0, 1e-9, 3, 40.0])
    A, R = np.meshgrid(a, res, indexing="ij")
    got = od_np.log_pf(R, A)
    want = scipy.stats.f.logsf(np.exp(R), 2 * A, 2 * A)
    ok = np.isfinite(want)
    assert ok.sum() >= 25
    err = np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))
    assert err.max() < 1e-9, err.max()
    assert od_np.log_pf_one(-np.inf, 3.0) == 0.0 and math.isnan(od_np.log_pf_one(1.0, 0.0)) and math.isnan(od_np.log_pf_one(np.nan, 2.0))
    assert od_np.log_pf_one(0.0, 30000.0) == math.log(0.5)                          # the median of F(d, d) is 1
    assert -2.2e7 < od_np.log_pf_one(700.0, 3e4) < -2.0e7                           # about a * (-res)


def test_log_qchisq_is_scipys_chi_square_quantile_above_minus_700():
    lp = np.array([-1e-12, -0.1, -1, -50, -690.0])
    for df in (1, 2, 199, 53999):
        got = od_np.log_qchisq(lp, df)
        want = scipy.stats.chi2.isf(np.exp(lp), df)
        want[0] = scipy.stats.chi2.ppf(-np.expm1(lp[0]), df)      # exp(-1e-12) rounds 1 - 1e-12 to 1e-4 of its distance from 1
        np.testing.assert_allclose(got, want, rtol=2e-9, err_msg=str(df))
    np.testing.assert_allclose(od_np.log_qchisq(np.array([-5000.0, -700.0]), 2), [10000.0, 1400.0], rtol=1e-15)   # Q(1, y) = exp(-y)
    assert od_np.log_qchisq_one(0.0, 5) == 0.0 and od_np.log_qchisq_one(-np.inf, 5) == np.inf
    assert all(math.isnan(od_np.log_qchisq_one(l, d)) for l, d in ((0.5, 5), (np.nan, 5), (-1.0, 0)))
    # both branches of log Q meet
    for a in (0.5, 99.5, 26999.5):
        lo, hi = od_np.log_Q(a, a + 1 - 1e-9), od_np.log_Q(a, a + 1 + 1e-9)
        assert abs(lo - hi) < 1e-8 and lo > hi


def test_bh_adjust_log_is_p_adjust_where_nothing_underflows():
    rng = np.random.default_rng(2)
    p = np.concatenate([rng.uniform(size=300) ** 4, [1.0, 1e-300, 0.2, 0.2, 0.2]])
    lp = np.log(p)
    lp[[5, 17]] = np.nan
    got = od_np.bh_adjust_log(lp)
    keep = ~np.isnan(lp)
    assert np.isnan(got[~keep]).all()
    np.testing.assert_allclose(got[keep], np.log(gficf_amd.p_adjust_fdr(p[keep])), rtol=1e-12, atol=1e-12)
    # R's bh.adjust does not cap at log(1): the largest adjusted value is the largest lp itself
    assert got[keep].max() == lp[keep].max()


def test_scale_factor_and_selection_rule():
    qv = np.array([5.0, 1e-9, 1e9, np.nan, 2.0, 3.0])
    v = np.array([0.0, 0.0, 0.0, 0.0, -np.inf, np.log(3.0)])
    np.testing.assert_allclose(od_np.gsf(qv, v), [math.sqrt(5), math.sqrt(1e-3), math.sqrt(1e3), 0.0, 0.0, 1.0])
    lp = np.array([-9.0, -1.0, np.nan, -7.0, -8.0, -0.5, -6.0])
    lpa = np.array([-5.0, -0.1, np.nan, -4.0, -4.5, -0.01, -3.0])
    for fn in (od_np.odgenes_rows, lambda a, b, n=None: gficf_amd.odgenes_rows({"lp": a, "lpa": b}, n)):
        np.testing.assert_array_equal(fn(lp, lpa), [0, 3, 4, 6])
        np.testing.assert_array_equal(fn(lp, lpa, 2), [0, 3])                        # the first two in row order, not the two smallest
        np.testing.assert_array_equal(fn(lp, lpa, 4), [0, 3, 4, 6])
        np.testing.assert_array_equal(fn(lp, lpa, 5), [0, 1, 3, 4, 6])               # more than significant: by lp
        np.testing.assert_array_equal(fn(lp, lpa, 99), np.arange(7))                 # min(G, n): the NaN row last in, still in


def test_planted_fixture_selects_its_genes_with_a_margin():
    """The fixture of the end-to-end GPU test, checked with the oracle alone: no gene's lpa within 1e-6 of log(0.1) and at
    least 20 of the 25 planted genes selected."""
    X, hot = od_np.planted()
    assert X.shape == (300, 200) and len(hot) == 25 and (X.sum(axis=1) > 0).all()
    var, nobs = od_np.moments(X)
    w = np.log(201.0 / (nobs + 1.0))                                                 # the classic ICF weight of gficf()
    r = od_np.over_dispersed(w, var, nobs, 200)
    assert r["basis"] == 5 and r["valid"].all()
    assert np.abs(r["lpa"] - math.log(0.1)).min() > 1e-6
    sel = np.flatnonzero(r["lpa"] < math.log(0.1))
    assert len(np.intersect1d(sel, hot)) >= 20 and len(sel) <= 40
    assert (r["gsf"] > 0).all()


# ------------------------------------------------------------------ the argument handling of the Python mirror
def test_argument_errors():
    M = sp.random(30, 12, density=0.4, random_state=0, format="csc")
    data = {"gficf": M, "w": np.linspace(1, 3, 30)}
    for fn in (gficf_amd.runPCA, gficf_amd.runLSA):
        with pytest.raises(NotImplementedError, match="findOverDispersed") as e:
            fn(dict(data, rawCounts=M), dim=2, use_odgenes=True)
        assert 'use_odgenes="cr"' in str(e.value) and 'var_scale="cr"' in str(e.value)
        with pytest.raises(NotImplementedError, match='var_scale="cr"'):
            fn(dict(data), dim=2, var_scale=True)
        with pytest.raises(ValueError, match="Raw Counts absent"):
            fn(dict(data), dim=2, use_odgenes="cr")
        with pytest.raises(ValueError, match="Raw Counts absent"):
            fn(dict(data), dim=2, var_scale="cr")
        with pytest.raises(ValueError, match='must be False or "cr"'):
            fn(dict(data, rawCounts=M), dim=2, use_odgenes="tp")
    with pytest.raises(ValueError, match="Raw Counts absent"):
        gficf_amd.findOverDispersed(dict(data))
    with pytest.raises(NotImplementedError, match='basis="cr"'):
        gficf_amd.findOverDispersed(dict(data, rawCounts=M), basis="tp")
    with pytest.raises(NotImplementedError, match='basis="cr"'):
        gficf_amd.over_dispersed_from_moments([1.0], [1.0], [1], 5, basis="tp")
    with pytest.raises(ValueError, match="gam_k"):
        gficf_amd.over_dispersed_from_moments([1.0], [1.0], [1], 5, gam_k=2)
    with pytest.raises(ValueError, match="gam_k"):
        gficf_amd.over_dispersed_from_moments([1.0], [1.0], [1], 5, gam_k=9)
    with pytest.raises(ValueError, match="sp must be"):
        gficf_amd.over_dispersed_from_moments([1.0], [1.0], [1], 5, sp=-2)
    with pytest.raises(ValueError, match="one length"):
        gficf_amd.over_dispersed_from_moments([1.0, 2.0], [1.0, 2.0], [1], 5)
    with pytest.raises(ValueError, match="no row is selected"):
        gficf_amd.select_scale_rows(M, rows=[])
    with pytest.raises(ValueError, match="distinct rows"):
        gficf_amd.select_scale_rows(M, rows=[1, 1])
    with pytest.raises(ValueError, match="distinct rows"):
        gficf_amd.select_scale_rows(M, rows=[30])
    with pytest.raises(ValueError, match="one value per row"):
        gficf_amd.select_scale_rows(M, scale=np.ones(3))
    with pytest.raises(ValueError, match="one row per row of data\\['gficf'\\]"):
        gficf_amd.pca_project({"pca": {"gene_rows": np.arange(3), "odgenes": {"gsf": np.ones(30)}, "genes": np.zeros((3, 2))}}, M[:5])
