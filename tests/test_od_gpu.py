"""libgficf_od.so on the GPU against its oracle (tests/helpers/od_np.py): what a user acts on exactly (the selected sets, the
zeros of gsf, lpa from the device's own lp, the rows selected and scaled, the composition with rsvd and pca_project), the two
special functions and the fit to the rounding of their sums and library functions."""
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sp

import gficf_amd
from gficf_amd import GficfError
from tests.helpers import od_np

pytestmark = pytest.mark.gpu

# Largest deviations from the oracle measured on the MI355X over the inputs of this file (each test prints its own): lp absolute
# where |lp| <= 1 and relative beyond, qv and fit relative.  lp is the grid's a = 3e4 at res = 0, where terms of 4e4 cancel to
# log(1/2) (the fixtures, nobs <= 200, stay below 1.2e-13); qv the grid's df = 53 999, where terms of 3e5 cancel in log Q (the
# fixtures, df = 199, below 1e-14); fit the G = 5 000 case at sp = 1 (the others below 4e-13).  The round trip of log_qchisq
# through mpmath's log Q deviates by at most 9.63e-12 and is held to lp's bound.  Each bound is eight times its figure.
FIG = {"lp": 4.97e-11, "qv": 6.98e-14, "fit": 1.38e-11}
REL = {k: 8 * v for k, v in FIG.items()}
SP_FIXED = (1.0, 0.01)                                       # where the oracle's dense solve is itself well conditioned


def dev_lp(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    d = np.where(got == want, 0.0, d)
    return float(np.nanmax(d)) if d.size and np.isfinite(d).any() else 0.0


def dev_rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(got - want) / np.abs(want)
    d = np.where(got == want, 0.0, d)
    return float(np.nanmax(d)) if d.size and np.isfinite(d).any() else 0.0


def held(what, **figs):
    print(what, {k: f"{v:.3g}" for k, v in figs.items()})
    for k, v in figs.items():
        assert v <= REL[k], (what, k, v, REL[k])


def same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


# ------------------------------------------------------------------ the special functions on a grid
def test_log_pf_grid():
    A, R = np.meshgrid([0.5, 1, 2.5, 50, 1e3, 3e4], [-np.inf, -40, -3, -1e-9, 0, 1e-9, 3, 40, 700], indexing="ij")
    got = gficf_amd.log_pf(R, 2 * A)
    want = od_np.log_pf(R, A)
    assert (got[:, 0] == 0).all() and np.isfinite(got[:, 1:]).all() and (got <= 0).all()
    held("log_pf grid", lp=dev_lp(got, want))
    edge = gficf_amd.log_pf([1.0, -np.inf, np.nan, np.inf, -np.inf], [0.0, 0.0, 4.0, 4.0, 4.0])
    assert np.isnan(edge[:3]).all() and edge[3] == -np.inf and edge[4] == 0.0


def test_log_qchisq_grid():
    lp = np.array([0, -1e-12, -0.1, -1, -50, -700, -5000.0])
    for df in (1, 2, 199, 53999):
        got = gficf_amd.log_qchisq(lp, df)
        want = od_np.log_qchisq(lp, df)
        assert got[0] == 0.0 and (np.diff(got) > 0).all()
        # the round trip, by mpmath: log Q(df / 2, x / 2) = lp
        back = np.array([float(od_np.log_Q(df / 2.0, x / 2.0)) for x in got[1:]])
        held(f"log_qchisq df = {df}", qv=dev_rel(got, want), lp=dev_lp(back, lp[1:]))
    edge = gficf_amd.log_qchisq([np.nan, 0.5, -np.inf, 0.0], 7)
    assert np.isnan(edge[:2]).all() and edge[2] == np.inf and edge[3] == 0.0
    assert np.isnan(gficf_amd.log_qchisq([-1.0, 0.0], 0)).all()


# ------------------------------------------------------------------ from the moments
CASES = {"G1": (1, None, 0), "G6": (6, None, 0), "G7": (7, None, 0), "G8": (8, None, 0), "G257": (257, None, 0), "G5000": (5000, None, 0),
         "ties4": (300, 4, 0), "ties5": (300, 5, 0), "min_cells": (257, None, 40)}


@functools.lru_cache(maxsize=None)
def _case(name):
    G, ties, min_cells = CASES[name]
    m, var, nobs, N = od_np.moments_case(G, ties=ties)
    want = od_np.fit(m, var, nobs, min_gene_cells=min_cells)
    # lp and qv by mpmath on some 60 genes of a large case: an even stride, and every gene that is special
    special = np.flatnonzero((var == 0) | (nobs < 2) | ~want["valid"])
    want["picked"] = np.unique(np.concatenate([np.arange(0, G, max(1, G // 60)), special[:20]]))
    return m, var, nobs, N, min_cells, want


@pytest.mark.parametrize("name", sorted(CASES))
def test_over_dispersed_from_moments(name):
    m, var, nobs, N, min_cells, want = _case(name)
    G = len(m)
    got = gficf_amd.over_dispersed_from_moments(m, var, nobs, N, min_gene_cells=min_cells)
    assert np.array_equal(got["valid"], want["valid"]) and dev_rel(got["v"], want["v"]) <= 4.5e-16         # the last bit of log
    assert got["n"] == want["n"] and got["basis"] == want["basis"], (got["basis"], want["basis"])
    assert (got["res"][~want["valid"]] == -np.inf).all() and np.isnan(got["fit"][~want["valid"]]).all()
    assert (got["lp"][~want["valid"] & (nobs > 0)] == 0).all() and np.isnan(got["lp"][nobs == 0]).all()
    if want["basis"] >= 3:
        assert got["u"] == want["u"] and np.allclose(got["knots"], want["knots"], rtol=1e-15, atol=0)
        # the search: no worse a GCV score than the oracle's lambda, both scored by the oracle; the same edf
        vv = want["v"][want["valid"]]
        g_dev, edf_dev, _ = od_np.gcv_dense(want["X"], want["S"], vv, got["lambda"])
        g_or, edf_or, _ = od_np.gcv_dense(want["X"], want["S"], vv, want["lambda"])
        print(name, "lambda", got["lambda"], want["lambda"], "gcv", g_dev, g_or, "edf", got["edf"], edf_or)
        assert g_dev <= g_or * (1 + 1e-9)
        assert abs(got["edf"] - edf_dev) <= 1e-8 * edf_dev and abs(got["edf"] - edf_or) <= 1e-3
        # the fit at a fixed lambda
        for s in SP_FIXED:
            f_dev = gficf_amd.over_dispersed_from_moments(m, var, nobs, N, min_gene_cells=min_cells, sp=s)
            f_or = od_np.fit(m, var, nobs, min_gene_cells=min_cells, sp=s)
            assert f_dev["lambda"] == s
            held(f"{name} fit at sp = {s}", fit=dev_rel(f_dev["fit"], f_or["fit"]))
    elif want["n"] > 0:
        held(f"{name} line", fit=dev_rel(got["fit"], want["fit"]))
    # lp and qv against mpmath, on the device's own residuals (the search's lambda is the device's)
    pick = want["picked"]
    lp_or = np.array([od_np.log_pf_one(got["res"][g], nobs[g] / 2.0) for g in pick])
    qv_or = np.array([od_np.log_qchisq_one(got["lp"][g], N - 1) / N for g in pick])
    held(f"{name} scores", lp=dev_lp(got["lp"][pick], lp_or), qv=dev_rel(got["qv"][pick], qv_or))
    # lpa: the same adds and minima as the oracle's bh.adjust on the device's own lp, bit for bit; gsf from the device's qv
    assert same(got["lpa"], od_np.bh_adjust_log(got["lp"]))
    assert np.array_equal(got["gsf"] == 0, od_np.gsf(got["qv"], got["v"]) == 0) and np.allclose(got["gsf"], od_np.gsf(got["qv"], got["v"]), rtol=1e-14, atol=0)
    assert (got["gsf"][var == 0] == 0).all() and (got["gsf"][nobs == 0] == 0).all()
    # determinism
    again = gficf_amd.over_dispersed_from_moments(m, var, nobs, N, min_gene_cells=min_cells)
    assert all(same(got[k], again[k]) for k in ("v", "fit", "res", "lp", "lpa", "qv", "gsf")) and got["lambda"] == again["lambda"]


@pytest.mark.parametrize("n", [1, 2, 255, 257, 5000])
def test_bh_adjust_log_is_the_oracles_bit_for_bit(n):
    rng = np.random.default_rng(n)
    lp = np.log(rng.uniform(size=n) ** 6)
    if n > 2:
        lp[rng.integers(0, n, n // 4)] = lp[0]                # ties, broken by row
        lp[rng.integers(0, n, n // 10 + 1)] = np.nan
        lp[1] = -np.inf
        lp[2] = 0.0
    assert same(gficf_amd.bh_adjust_log(lp), od_np.bh_adjust_log(lp))
    assert np.isnan(gficf_amd.bh_adjust_log(np.full(n, np.nan))).all()


# ------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def _planted():
    X, hot = od_np.planted()
    data = gficf_amd.gficf(sp.csc_matrix(X), cell_proportion_min=0, normalize=False, verbose=False)
    assert np.array_equal(data["genes"], np.arange(300))
    var, nobs = od_np.moments(X)
    want = od_np.over_dispersed(np.asarray(data["w"], dtype=np.float64), var, nobs, 200)
    return X, hot, data, want


def test_findOverDispersed_on_the_planted_matrix(capsys):
    X, hot, data, want = _planted()
    st = gficf_amd.findOverDispersed(data, alpha=0.1, verbose=True, ret_stages=True)
    err = capsys.readouterr().err
    assert "calculating variance fit ..." in err and " using gam " in err and "overdispersed genes ..." in err and "done." in err
    t = st["table"]
    assert list(t.columns) == ["m", "v", "nobs", "res", "lp", "lpa", "qv", "gsf"] and len(t) == 300
    assert np.array_equal(t["nobs"], (X != 0).sum(axis=1)) and same(t["m"], data["w"])
    assert dev_rel(st["var"], X.var(axis=1, ddof=1)) < 1e-13
    assert np.abs(want["lpa"] - math.log(0.1)).min() > 1e-6                       # the fixture's margin, with the device's w
    sel = np.flatnonzero(want["lpa"] < math.log(0.1))
    assert np.array_equal(np.flatnonzero(t["lpa"] < math.log(0.1)), sel) and np.array_equal(st["ods"], sel)
    assert len(np.intersect1d(sel, hot)) >= 20
    assert np.array_equal(t["gsf"].to_numpy() == 0, want["gsf"] == 0)
    assert np.array_equal(gficf_amd.odgenes_rows(t), od_np.odgenes_rows(want["lp"], want["lpa"]))
    assert st["basis"] == 5 and st["n"] == 300
    # the table is the moments call fed the matrix call's own moments, and the same on every call
    fm = gficf_amd.over_dispersed_from_moments(data["w"], st["var"], t["nobs"].to_numpy(), 200)
    t2 = gficf_amd.findOverDispersed(data, verbose=False)
    for k in ("v", "res", "lp", "lpa", "qv", "gsf"):
        assert same(fm[k], t[k]) and same(t2[k], t[k]), k
    lo = gficf_amd.findOverDispersed(data, verbose=False, use_unadjusted_pvals=True, alpha=0.05, ret_stages=True)
    assert np.array_equal(lo["ods"], np.flatnonzero(t["lp"] < math.log(0.05)))


# ------------------------------------------------------------------ rows selected and scaled
def _sparse(G, N, seed, dtype):
    rng = np.random.default_rng(seed)
    M = sp.random(G, N, density=0.3, random_state=seed, format="csc")
    M.data[:] = rng.uniform(0.1, 2.0, len(M.data))
    if N > 2:
        M = sp.csc_matrix(M.toarray() * (np.arange(N) % 7 != 3)[None, :])         # empty columns
    M.indptr, M.indices = M.indptr.astype(dtype), M.indices.astype(np.int32)
    return M


@pytest.mark.parametrize("N", [1, 255, 1025])
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_select_scale_rows_is_scipys(N, dtype):
    G = 67
    M = _sparse(G, N, N, dtype)
    rng = np.random.default_rng(N)
    scale = rng.uniform(0.5, 2.0, G)
    scale[::5] = 0.0                                                               # stay stored, as 0
    dense = M.toarray()
    some = np.sort(rng.choice(G, 20, replace=False))
    lonely = np.flatnonzero(dense[:, min(1, N - 1)] == 0)[:10]                     # a column that loses all its entries
    for rows in (some, lonely, np.arange(G), np.array([G - 1])):
        for sc in (None, scale):
            got = gficf_amd.select_scale_rows(M, rows, sc)
            ref = M.tocsr()[rows].tocsc()                                          # M[rows].multiply(scale[rows][:, None]): one product
            ref.sort_indices()
            assert got.shape == (len(rows), N) and np.array_equal(got.indptr, ref.indptr) and np.array_equal(got.indices, ref.indices)
            assert same(got.data, ref.data if sc is None else ref.data * sc[rows][ref.indices])
    got = gficf_amd.select_scale_rows(M, None, scale)
    assert got.shape == M.shape and np.array_equal(got.indptr, M.indptr) and np.array_equal(got.indices, M.indices)
    assert same(got.data, M.data * scale[M.indices]) and got.nnz == M.nnz
    assert same(gficf_amd.select_scale_rows(M, some[::-1], None).toarray(), dense[some])    # ascending, whatever the order asked in
    with pytest.raises(ValueError, match="no row is selected"):
        gficf_amd.select_scale_rows(M, [], scale)


def test_select_scale_rows_refuses_a_bad_matrix():
    M = _sparse(20, 30, 0, np.int32)
    bad = sp.csc_matrix((M.data, M.indices.copy(), M.indptr), shape=M.shape)
    bad.indices[3] = 25
    bad.has_sorted_indices = True
    with pytest.raises(GficfError) as e:
        gficf_amd.select_scale_rows(bad, [0, 1], None)
    assert "out of range" in str(e.value)
    assert gficf_amd.select_scale_rows(M, [0, 1], None).shape == (2, 30)             # the status word was cleared


# ------------------------------------------------------------------ runPCA, runLSA, embedNewCells
@pytest.mark.parametrize("fn", ["runPCA", "runLSA"])
def test_decomposition_is_rsvd_of_the_selected_scaled_matrix(fn):
    _, _, data, want = _planted()
    run = getattr(gficf_amd, fn)
    table = gficf_amd.findOverDispersed(data, alpha=0.1, verbose=False)
    sig = od_np.odgenes_rows(want["lp"], want["lpa"])
    assert np.array_equal(gficf_amd.odgenes_rows(table), sig) and len(sig) >= 20
    gsf = table["gsf"].to_numpy()
    centre = fn == "runPCA"
    for use, scale, n_od in (("cr", False, None), (False, "cr", None), ("cr", "cr", None), ("cr", "cr", 10), ("cr", False, len(sig) + 15)):
        rows = od_np.odgenes_rows(want["lp"], want["lpa"], n_od) if use else np.arange(300)
        if n_od == 10:
            assert np.array_equal(rows, sig[:10])                                  # below the significant count: the first in row order
        elif n_od:
            assert len(rows) == len(sig) + 15 and np.array_equal(rows, np.sort(np.argsort(table["lp"].to_numpy(), kind="stable")[:len(rows)]))
        d = run(dict(data), dim=4, use_odgenes=use, var_scale=scale, n_odgenes=n_od, centre=centre, plot_odgenes=False)
        M = gficf_amd.select_scale_rows(data["gficf"], rows if use else None, gsf if scale else None)
        r = gficf_amd.rsvd(M, 4, centre=centre)
        assert np.array_equal(d["pca"]["gene_rows"], rows) and d["pca"]["genes"].shape == (len(rows), 4) and d["pca"]["rescale"] is bool(scale)
        assert same(d["pca"]["cells"], r["cells"]) and same(d["pca"]["genes"], r["v"]), (use, scale, n_od)
        assert all(same(d["pca"]["odgenes"][k], table[k]) for k in table.columns)
    with pytest.warns(UserWarning, match="plot_odgenes"):
        run(dict(data), dim=2, use_odgenes="cr", plot_odgenes=True)


def test_embedNewCells_selects_and_scales_the_new_cells():
    X, _, data, _ = _planted()
    Xs = sp.csc_matrix(X)
    d = gficf_amd.runPCA(dict(data), dim=14, use_odgenes="cr", var_scale="cr", n_odgenes=24)   # l = min(14 + 10, 24): every direction
    rows, gsf = d["pca"]["gene_rows"], d["pca"]["odgenes"]["gsf"].to_numpy()
    assert len(rows) == 24
    d = gficf_amd.runReduction(d, n_epochs=20, verbose=False)
    d = gficf_amd.embedNewCells(d, Xs, verbose=False)
    # by hand: the new cells' GF-ICF, the rows picked and scaled, projected
    g, kept = gficf_amd.gficf_with_weights(Xs, data["w"])
    g = sp.csc_matrix((g.data, kept[g.indices].astype(np.int32), g.indptr), shape=(300, 200))
    hand = sp.csc_matrix(g.tocsr()[rows].multiply(gsf[rows][:, None]))
    want = gficf_amd.pca_project({"pca": {"genes": d["pca"]["genes"], "centre": False}}, hand)
    assert same(d["pca"]["pred"], want)
    # the training cells embedded again are the training cells (the bound tests/test_pca_gpu.py holds the closed forms to)
    d0 = np.linalg.norm(d["pca"]["cells"], axis=0)[0]
    assert np.abs(d["pca"]["pred"] - d["pca"]["cells"]).max() <= 1e-12 * d0
    assert (d["embedded"]["predicted"] == "YES").sum() == 200


def test_the_old_paths_are_unchanged():
    _, _, data, _ = _planted()
    for fn, centre in ((gficf_amd.runPCA, True), (gficf_amd.runLSA, False)):
        d = fn(dict(data), dim=5, centre=centre)
        assert set(d["pca"]) == {"cells", "genes", "centre", "rescale", "mean"} and d["pca"]["rescale"] is False
        r = gficf_amd.rsvd(data["gficf"], 5, centre=centre)
        assert same(d["pca"]["cells"], r["cells"]) and same(d["pca"]["genes"], r["v"])
        M = data["gficf"][:, :40]
        lib = {"genes": d["pca"]["genes"], "centre": d["pca"]["centre"], "mean": d["pca"]["mean"]}
        assert same(gficf_amd.pca_project(d, M), gficf_amd.pca_project({"pca": lib}, M))


def test_device_resident_chain_is_the_host_call():
    X, _, data, _ = _planted()
    table = gficf_amd.findOverDispersed(data, alpha=0.1, verbose=False, ret_stages=True)
    ops = gficf_amd.HipOps(0)
    tc = ops.torch
    dev = tc.device("cuda", 0)
    t = lambda a, dt: tc.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    G, N = 300, 200
    M = data["gficf"]
    f64 = lambda n: tc.empty(n, dtype=tc.float64, device=dev)
    ws = tc.zeros(ops.od_workspace_bytes(G, N), dtype=tc.uint8, device=dev)
    v, fit, res, lp, lpa, qv, gsf = (f64(G) for _ in range(7))
    valid = tc.empty(G, dtype=tc.int32, device=dev)
    nobs = t(table["table"]["nobs"].to_numpy(), np.int32)
    info = ops.od_fit(t(data["w"], np.float64), t(table["var"], np.float64), nobs, ws, v, valid, fit, res)
    ops.od_scores(res, nobs, v, N, ws, lp, qv, gsf)
    ops.od_bh_log(lp, ws, lpa)
    mask = (lpa < math.log(0.1)).to(tc.int32)
    colptr, rowidx, x = t(M.indptr, np.int64), t(M.indices, np.int32), t(M.data, np.float64)
    ocp, orow, ox = tc.empty(N + 1, dtype=tc.int64, device=dev), tc.empty(M.nnz, dtype=tc.int32, device=dev), f64(M.nnz)
    nsel = tc.empty(1, dtype=tc.int32, device=dev)
    ops.od_select_scale(G, N, colptr, rowidx, x, mask, gsf, ws, ocp, orow, ox, nsel)
    ops.od_sync(ws)
    assert info["lambda"] == table["lambda"] and info["basis"] == 5
    for name, dv in (("v", v), ("res", res), ("lp", lp), ("lpa", lpa), ("qv", qv), ("gsf", gsf)):
        assert same(dv.cpu().numpy(), table["table"][name]), name
    rows = gficf_amd.odgenes_rows(table["table"])
    want = gficf_amd.select_scale_rows(M, rows, table["table"]["gsf"].to_numpy())
    n_out = int(ocp[-1])
    assert int(nsel[0]) == len(rows) and n_out == want.nnz and np.array_equal(ocp.cpu().numpy(), want.indptr)
    assert np.array_equal(orow[:n_out].cpu().numpy(), want.indices) and same(ox[:n_out].cpu().numpy(), want.data)
    # ... and on into rsvd without leaving the device
    Gs, k, l = len(rows), 4, 14
    om = np.random.default_rng(180582).standard_normal((min(N, Gs), l))
    ws2 = tc.empty(ops.rsvd_workspace_bytes(Gs, N, n_out, l), dtype=tc.uint8, device=dev)
    d, cells, genes = f64(k), tc.empty((k, N), dtype=tc.float64, device=dev), tc.empty((k, Gs), dtype=tc.float64, device=dev)
    ops.rsvd(Gs, N, ocp, orow[:n_out].contiguous(), ox[:n_out].contiguous(), False, t(np.asfortranarray(om).T, np.float64), k, l, 2, ws2, d, cells, genes)
    ops.rsvd_sync(ws2)
    r = gficf_amd.rsvd(want, k, omega=om)
    assert same(cells.cpu().numpy().T, r["cells"]) and same(genes.cpu().numpy().T, r["v"])
