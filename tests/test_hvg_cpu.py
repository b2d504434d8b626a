"""No GPU: the NumPy oracle of libgficf_hvg.so (tests/helpers/hvg_np.py, the yardstick of tests/test_hvg_gpu.py) against
answers derived by hand, on a planted trend and where the trend cannot be fitted; the header against its loader and the
Makefile; the argument handling of the Python mirror."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import gficf_amd
from gficf_amd import synth
from tests.helpers import hvg_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_loader_name_the_same_entries():
    from gficf_amd import _hvg_lib

    text = open(os.path.join(ROOT, "include", "gficf_hvg.h")).read()
    body = text[text.index("extern \"C\""):]
    declared = re.findall(r"\b(gficf_hvg_\w+)\s*\(([^;]*)\)\s*;", body)
    assert set(n for n, _ in declared) == set(_hvg_lib.SIGNATURES) and len(declared) == 12
    for name, args in declared:
        n = 0 if args.strip() == "void" else args.count(",") + 1
        assert n == len(_hvg_lib.SIGNATURES[name][1]), name
    assert "#define GFICF_HVG_ABI_VERSION 1" in text and _hvg_lib.ABI_VERSION == 1
    for macro, value in (("KDE_N", _hvg_lib.KDE_N), ("GRID5_MAX", _hvg_lib.GRID5_MAX), ("GRID1_MAX", _hvg_lib.GRID1_MAX), ("SCALARS", len(_hvg_lib.SCALARS))):
        assert re.search(rf"#define\s+GFICF_HVG_{macro}\s+{value}\b", text), macro
    # the longest grids finite positive doubles can ask for
    span = np.log10(np.finfo(np.float64).max) - np.log10(5e-324)
    assert hvg_np.seq_len(0.0, span, 0.005) <= _hvg_lib.GRID5_MAX and hvg_np.seq_len(0.0, span, 0.001) <= _hvg_lib.GRID1_MAX
    core = open(os.path.join(ROOT, "include", "gficf_hip.h")).read()
    assert re.search(r"#define\s+GFICF_HIP_ABI_VERSION\s+7\b", core)


def test_makefile_builds_the_library_with_the_others():
    csrc = os.path.join(ROOT, "gficf_amd", "csrc")
    build = subprocess.run(["make", "-n", "-B", "-C", csrc, "all"], capture_output=True, text=True, check=True).stdout.splitlines()
    link = [ln for ln in build if " -o ../libgficf_hvg.so " in ln]
    assert len(link) == 1 and re.search(r"hipcc --offload-arch=gfx950 -shared -fPIC -o \.\./libgficf_hvg\.so hvg\.o -L\.\. -lgficf_hip\b", link[0])
    comp = [ln for ln in build if ln.endswith(" -o hvg.o")]
    assert len(comp) == 1 and "-ffp-contract=off" in comp[0] and "--offload-arch=gfx950" in comp[0] and "fast-math" not in comp[0]
    assert build.index(link[0]) > max(i for i, ln in enumerate(build) if " -o ../libgficf_hip.so " in ln or ln.endswith(" -o hvg.o"))
    clean = subprocess.run(["make", "-n", "-C", csrc, "clean"], capture_output=True, text=True, check=True).stdout
    assert re.search(r"^rm -f .*\bhvg\.o\b.* \.\./libgficf_hvg\.so\b", clean, re.M)


def test_loader(monkeypatch):
    from gficf_amd import _hvg_lib

    L = _hvg_lib.load()
    assert isinstance(L, ctypes.CDLL) and _hvg_lib.load() is L and L.gficf_hvg_abi_version() == _hvg_lib.ABI_VERSION
    for sym, (res, args) in _hvg_lib.SIGNATURES.items():
        fn = getattr(L, sym)
        assert fn.restype is res and list(fn.argtypes) == list(args), sym
    assert os.path.basename(_hvg_lib.LIB_PATH) == "libgficf_hvg.so"
    lists = L.gficf_hvg_workspace_bytes(23000, 0, 0, 0)
    assert 100 * 23000 < lists < 200 * 23000
    assert L.gficf_hvg_workspace_bytes(23000, 54000, 60_000_000, 0) >= lists + 12 * 60_000_000
    assert L.gficf_hvg_workspace_bytes(23000, 0, 0, 4001) >= lists + 36 * 4001 - 4096
    assert L.gficf_hvg_workspace_bytes(0, 0, 0, 0) == 0 and L.gficf_hvg_workspace_bytes(10, 0, 0, _hvg_lib.GRID1_MAX + 1) == 0
    monkeypatch.setattr(_hvg_lib, "LIB_PATH", os.path.join(os.path.dirname(_hvg_lib.LIB_PATH), "libgficf_hvg_missing.so"))
    with pytest.raises(ImportError, match="not found: build it with"):
        _hvg_lib.load()


# ------------------------------------------------------------------ the oracle against what defines it
def test_moments_are_numpys_on_the_dense_matrix():
    rng = np.random.default_rng(0)
    X = rng.poisson(0.8, (40, 57)).astype(np.float64)
    X[3], X[4] = 0, 2.0
    m = hvg_np.moments(X)
    np.testing.assert_allclose(m["mean"], X.mean(axis=1), rtol=1e-14)
    np.testing.assert_allclose(m["sd"], X.std(axis=1, ddof=1), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(m["var"], X.var(axis=1, ddof=1), rtol=1e-12, atol=1e-15)
    assert np.array_equal(m["nobs"], (X != 0).sum(axis=1))
    assert not m["valid"][3] and not m["valid"][4] and m["valid"].sum() == 38 and m["sd"][4] == 0


def test_local_fit_returns_a_quadratic_exactly():
    rng = np.random.default_rng(1)
    x = np.sort(rng.uniform(-2, 5, 120))
    quad = lambda v: (0.7 - 1.3 * v + 0.4 * v * v) / 5                     # |y| <= 1 on the data
    y = quad(x)
    at = np.concatenate([x[::7], np.linspace(-2.1, 5.1, 23), [x[0], x[-1]]])      # at the data, between, beyond both ends
    holes = np.where(rng.random(120) < .3, 0.0, 1.0)                      # zero weights: a window needs three weighted points
    for w in (None, rng.uniform(0.1, 3, 120), holes):
        for k in (8, 24, 120):
            if w is holes and k == 8:
                continue                                                  # two weighted points do not determine a quadratic
            got = hvg_np.local_fit(x, y, at, k, w)
            assert np.abs(y).max() <= 1 and np.abs(got - quad(at)).max() <= 1e-12, (k, w is None)


def test_local_fit_is_a_weighted_polyfit_over_the_window():
    rng = np.random.default_rng(2)
    n, k = 90, 18
    x = rng.uniform(0, 4, n)
    y = np.sin(2 * x) + 0.1 * rng.standard_normal(n)
    w = rng.uniform(0.2, 2, n)
    for x0 in (x[5], 0.0, 2.22, 4.0):
        d = np.abs(x - x0)
        h = np.sort(d)[k - 1]
        W = np.where(d < h, (1 - (d / h) ** 3) ** 3, 0.0) * w
        keep = W > 0
        want = np.polyval(np.polyfit(x[keep] - x0, y[keep], 2, w=np.sqrt(W[keep])), 0.0)
        got, hh = hvg_np.local_fit(x, y, [x0], k, w, ret_h=True)
        assert hh[0] == h and got[0] == pytest.approx(want, rel=1e-10, abs=1e-12)
    # fewer distinct x than the degree needs: the degree is lowered, not divided by a vanishing pivot
    assert hvg_np.local_fit([1.0, 1.0, 2.0, 2.0, 9.0], [1.0, 3.0, 4.0, 6.0, 0.0], [1.5], 5)[0] == pytest.approx(3.5, rel=1e-12)
    assert np.isnan(hvg_np.local_fit([1.0, 1.0, 2.0, 2.0, 9.0], [1.0, 3.0, 4.0, 6.0, 0.0], [1.5], 4)[0])    # all four at distance h
    assert hvg_np.local_fit([1.0, 1.0, 1.0, 5.0], [1.0, 2.0, 6.0, 0.0], [1.0], 3)[0] == pytest.approx(3.0, rel=1e-15)        # h = 0
    assert np.isnan(hvg_np.local_fit([1.0, 2.0, 3.0, 9.0], [1.0, 2.0, 3.0, 4.0], [2.0], 3, [0.0, 0.0, 0.0, 1.0])[0])


def test_robust_weights_are_clevelands():
    res = np.array([0.0, 0.3, -0.6, 3.0, -6.0, 7.0])
    assert hvg_np.r_median([3.0, 1.0, 2.0]) == 2.0 and hvg_np.r_median([4.0, 1.0, 2.0, 3.0]) == 2.5
    np.testing.assert_allclose(hvg_np.bisquare(res, 1.0), [1.0, (1 - .0025) ** 2, (1 - .01) ** 2, .75 ** 2, 0.0, 0.0], rtol=1e-15)
    x = np.linspace(0, 1, 60)
    y = 1 + 2 * x
    fit, w, s = hvg_np.robust_fit(x, np.zeros(60), 12)                    # an exact fit: s = 0 stops the loop at once
    assert (fit == 0).all() and (w == 1).all() and (s == 0).all()
    y2 = y + 0.05 * np.random.default_rng(3).standard_normal(60)
    y2[30] += 1.0                                                         # one outlier loses its weight
    fit, w, s = hvg_np.robust_fit(x, y2, 12)
    assert w[30] == 0 and (w > 0).sum() >= 55 and (s > 0).all() and abs(fit[30] - y[30]) < 0.1
    plain = hvg_np.local_fit(x, y2, x, 12)
    assert abs(plain[30] - y[30]) > 2 * abs(fit[30] - y[30])


def test_seq_has_rs_length():
    assert hvg_np.seq_len(0, 1, 0.1) == 11 and hvg_np.seq_len(0, 0.3, 0.1) == 4           # 0.3 / 0.1 = 2.9999999999999996
    assert hvg_np.seq_len(0, 0.999, 0.005) == 200 and hvg_np.seq_len(0, 1, 0.005) == 201 and hvg_np.seq_len(2, 2, 0.005) == 1
    assert hvg_np.seq_len(-1.2345, 3.2105, 0.001) == 4446
    g = hvg_np.seq(-1.2345, 3.2105, 0.001)
    assert g[0] == -1.2345 and g[1] == -1.2345 + 0.001 and g[-1] <= 3.2105 + 1e-9 and len(g) == 4446
    assert list(hvg_np.gap_counts([0.0, 0.05, 0.0999, 0.1, 0.3], [0.05, 0.15])) == [3, 1]      # [0, 0.1) and [0.1, 0.2)


def test_trusted_range_rules():
    g5 = hvg_np.seq(-1, 1, 0.005)
    gap = np.full(len(g5), 3)
    gap[50:] = 9
    y = -g5.copy()
    assert hvg_np.trusted_range(1000, g5, gap, y) == (50, len(g5) - 2)               # no rise: the fall-back
    y[300:] += 0.02 * np.arange(1, len(g5) - 299)                                    # rises from 299 -> 300 on, where g5 > 0
    assert g5[300] > 0 and hvg_np.trusted_range(1000, g5, gap, y) == (50, 299)
    y[100:120] += 1.0                                                                # a rise where g5 <= 0 does not count
    assert g5[120] <= 0 and hvg_np.trusted_range(1000, g5, gap, y) == (50, 299)
    for bad_gap, G in ((np.full(len(g5), 3), 1000), (gap, 2000)):
        with pytest.raises(ValueError, match="cannot be fitted"):
            hvg_np.trusted_range(G, g5, bad_gap, y)
    gap[:] = 3
    gap[298:] = 9
    with pytest.raises(ValueError, match="cannot be fitted"):                        # two points
        hvg_np.trusted_range(1000, g5, gap, y)


def test_nls_recovers_a_curve():
    x = 10.0 ** np.linspace(0, 3, 40)
    for b, a in ((37.5, 0.08), (1.0e4, 0.07), (2.0, 1.5)):
        gb, ga, it = hvg_np.nls(x, hvg_np.curve(x, b, a))
        assert gb == pytest.approx(b, rel=1e-9) and ga == pytest.approx(a, rel=1e-9) and 2 <= it <= 50
    with pytest.raises(ValueError, match="cannot be fitted.*singular"):             # one x: b and a cannot be told apart
        hvg_np.nls(np.full(5, 10.0), np.array([0.1, 0.2, 0.15, 0.1, 0.2]))


def test_distance_signs_by_hand():
    # the curve b = 1, a = 0 is the line y = -g / 2.  lx, ly, the nearest grid index, the sign
    line = lambda g: -0.5 * g
    table = [(0.0, line(0.0) + 0.05, 0, +1),                  # at the left end, above: its own grid point (not to its right)
             (1.0, line(1.0) - 0.05, 1000, -1),               # at the right end, below: the last grid point, which is not above it
             (0.5004, line(0.5004) + 0.1, 460, +1),           # above: the foot of the perpendicular lies 0.04 to the left
             (0.5004, line(0.5004) - 0.1, 540, -1),           # below: 0.04 to the right
             (0.4999, line(0.4999) + 0.0002, 500, -1),        # just above, the point to its right nearest: the overwritten branch
             (0.5001, line(0.5001) - 0.0002, 500, -1),        # just below, the point to its left nearest
             (0.0 + 300 * 0.001, line(0.3) + 1e-5, 300, +1)]  # on a grid point, a hair above it
    lx, ly = np.array([t[0] for t in table]), np.array([t[1] for t in table])
    cv, index, sign, margin = hvg_np.curve_distance(lx, ly, 1.0, 0.0, ret_all=True)
    assert list(index) == [t[2] for t in table] and list(sign) == [t[3] for t in table] and margin.min() > 1e-9
    g1 = hvg_np.seq(0.0, 1.0, 0.001)
    right, above = g1[index] > lx, line(g1[index]) < ly
    assert {(bool(r), bool(u)) for r, u in zip(right, above)} == {(True, True), (True, False), (False, True), (False, False)}
    d = np.sqrt((g1[index] - lx) ** 2 + (line(g1[index]) - ly) ** 2)
    np.testing.assert_allclose(cv, sign * d * np.log2(10.0), rtol=1e-9)
    assert d[2] == pytest.approx(0.1 / np.sqrt(1.25), rel=1e-4) and d[6] == pytest.approx(1e-5, rel=1e-6)


def test_bandwidth_by_hand():
    v = np.array([1.0, 2, 3, 4, 5, 6, 7, 8, 9, 100])                     # quartiles 3.25 and 7.75; sd far above IQR / 1.34
    assert hvg_np.bw_nrd0(v) == pytest.approx(0.9 * (4.5 / 1.34) * 10 ** -0.2, rel=1e-14)
    v = np.array([0.0, 1.0, 2.0, 3.0, 4.0])                              # sd = sqrt(2.5) = 1.58 below IQR / 1.34 = 1.49? no: min is 1.49
    assert hvg_np.bw_nrd0(v) == pytest.approx(0.9 * min(np.sqrt(2.5), 2 / 1.34) * 5 ** -0.2, rel=1e-14)
    assert hvg_np.bw_nrd0(np.array([1.0, 1, 1, 1, 9])) == pytest.approx(0.9 * np.std([1, 1, 1, 1, 9], ddof=1) * 5 ** -0.2, rel=1e-14)   # IQR = 0 -> sd
    assert hvg_np.bw_nrd0(np.array([-2.0, -2, -2])) == pytest.approx(0.9 * 2 * 3 ** -0.2, rel=1e-14)                                 # sd = 0 -> |x1|
    assert hvg_np.bw_nrd0(np.zeros(4)) == pytest.approx(0.9 * 4 ** -0.2, rel=1e-14)                                                 # -> 1
    bw, grid, dens = hvg_np.density(np.array([0.0, 0.0, 0.0, 0.1, 4.0]))
    assert len(grid) == 512 and grid[0] == -3 * bw and grid[-1] == 4 + 3 * bw and abs(grid[int(np.argmax(dens))]) < 0.1


def test_pvalues_by_hand():
    cv = np.array([-0.2, -0.1, 0.0, 0.1, 3.0])
    mu, sigma, P = hvg_np.pvalues(cv, 0.0)                                # tmp = -0.2, -0.1, 0, 0.2, 0.1
    assert mu == pytest.approx(0.0, abs=1e-16) and sigma == pytest.approx(np.sqrt(0.1 / 5), rel=1e-14)
    assert P[2] == pytest.approx(0.5, rel=1e-15) and P[0] > 0.5 > P[3] > P[4] and P[4] < 1e-90
    assert np.allclose(hvg_np.p_adjust_fdr(P), gficf_amd.p_adjust_fdr(P), rtol=0, atol=0)
    fdr = np.array([.5, np.nan, .01, .5, .02])
    assert list(hvg_np.select_rows(fdr)) == [2, 4, 0, 3, 1] and list(gficf_amd.hvg_rows(fdr)) == [2, 4, 0, 3, 1]
    many = np.concatenate([np.full(1001, .05), np.full(10, .5)])
    assert len(gficf_amd.hvg_rows(many)) == 1001 and len(gficf_amd.hvg_rows(many[1:])) == 1000


# ------------------------------------------------------------------ planted data
@pytest.mark.parametrize("G,seed,cut", [(400, 1, True), (150, 2, True), (1000, 3, False)])
def test_planted_trend_is_recovered(G, seed, cut):
    mean, cv, up = hvg_np.planted(G, seed)
    r = hvg_np.var_genes_from_moments(mean, cv)
    print(f"G={G} seed={seed}: b={r['b']:.4f} a={r['a']:.5f} rounds={r['nls_iter']} cdx0={r['cdx0']} j0={r['j0']} of {len(r['g5'])} "
          f"found {int((r['P'][up] < .05).sum())}/{len(up)}")
    assert len(up) == G // 20 and abs(r["b"] / 50 - 1) < .1 and abs(r["a"] / .05 - 1) < .1
    assert (r["P"][up] < .05).all()
    if cut:                                                               # a rise inside the grid ends the range, not the fall-back
        assert r["j0"] < len(r["g5"]) - 2
    assert r["valid"].all() and np.isfinite(r["FDR"]).all() and (r["weights"] >= 0).all() and (r["weights"][up] < 0.5).mean() > 0.8


def test_a_trend_that_cannot_be_fitted_is_an_error():
    colptr, rowidx, x = synth.counts_csc(600, 120, 0.07, seed=3)
    X = sp.csc_matrix((x, rowidx, colptr), shape=(600, 120)).toarray()
    X = X / (1e-6 * X.sum(axis=0))[None, :]
    with pytest.raises(ValueError, match="the variance-mean trend cannot be fitted"):
        hvg_np.find_var_genes(X)


# ------------------------------------------------------------------ the mirror's argument handling
def test_argument_errors():
    with pytest.raises(ValueError, match="at least 20"):
        gficf_amd.findVarGenes(sp.csc_matrix(np.ones((19, 6))))
    with pytest.raises(ValueError, match="at least 20"):
        gficf_amd.var_genes_from_moments(np.r_[np.ones(19), np.zeros(5)], np.ones(24))
    with pytest.raises(ValueError, match="at least 2 cells"):
        gficf_amd.findVarGenes(sp.csc_matrix(np.ones((30, 1))))
    with pytest.raises(ValueError, match="two cells"):
        gficf_amd.gene_moments(sp.csc_matrix(np.ones((30, 1))))
    with pytest.raises(NotImplementedError, match='"locfit"'):
        gficf_amd.findVarGenes(sp.csc_matrix(np.ones((30, 6))), fitMethod="loess")
    with pytest.raises(ValueError, match="one name per row"):
        gficf_amd.findVarGenes(sp.csc_matrix(np.ones((30, 6))), genes=["a"])
    with pytest.raises(ValueError, match="one length"):
        gficf_amd.var_genes_from_moments(np.ones(30), np.ones(29))
    with pytest.raises(ValueError, match="one length"):
        gficf_amd.local_regression(np.arange(10.0), np.arange(9.0))
    with pytest.raises(ValueError, match="finite"):
        gficf_amd.local_regression(np.r_[np.arange(9.0), np.nan], np.arange(10.0))
    with pytest.raises(ValueError, match="between 1 and all"):
        gficf_amd.local_regression(np.arange(10.0), np.arange(10.0), nn=0.05)
    with pytest.raises(ValueError, match="non-negative"):
        gficf_amd.local_regression(np.arange(10.0), np.arange(10.0), weights=-np.ones(10))
    with pytest.raises(ValueError, match="one length"):
        gficf_amd.curve_distance(np.ones(4), np.ones(5), 1.0, 0.0)
    data = {"community": np.array([1, 2]), "rawCounts": np.eye(2)}
    with pytest.raises(NotImplementedError, match="hvg=False") as e:
        gficf_amd.findClusterMarkers(dict(data), hvg=True)
    assert 'hvg="locfit"' in str(e.value) and "findVarGenes" in str(e.value)
    with pytest.raises(ValueError, match='"locfit", False or the row indices'):
        gficf_amd.findClusterMarkers(dict(data), hvg="loess")
    import inspect

    sig = inspect.signature(gficf_amd.findVarGenes).parameters
    assert list(sig)[:4] == ["cpms", "fitMethod", "verbose", "genes"] and sig["fitMethod"].default == "locfit"
    sig = inspect.signature(gficf_amd.local_regression).parameters
    assert list(sig)[:7] == ["x", "y", "at", "nn", "weights", "robust_iter", "ret_h"] and sig["nn"].default == 0.2
