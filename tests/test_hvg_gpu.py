"""libgficf_hvg.so on the GPU, stage by stage against its NumPy oracle (tests/helpers/hvg_np.py): what is a decision (valid,
nobs, h, the gap counts, the nearest grid point and the sign, the mode's grid index, cdx0, j0, the Gauss-Newton rounds, the
selected rows) exactly, what is a sum or a library function to the rounding of its order; the whole procedure; the Python
mirror."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import gficf_amd
from gficf_amd import synth
from tests.helpers import hvg_np

pytestmark = pytest.mark.gpu

# Largest relative differences to the oracle measured on the MI355X over the inputs of this file (each test prints its own).
# They come from the order of the sums and the last bit of log10, pow, exp and erfc; a neighbour more or fewer in a window or
# another grid point would show at 1e-4 and above.  Each bound is eight times its figure; none may exceed 1e-9 (P: 1e-8).
# The local fit on given points has no figure: the oracle adds in the kernel's order and the values are compared bit for bit
# (so are the three s and the weights of the robust loop).  In the whole procedure lx and ly come from the device's log10, a
# last bit off NumPy's, and the fit follows them: s, fit, ySeq and weights (absolute: they end at 0) have figures there.
#   moments (67 x 193, and the 1 993 x 300 counts per million): sd 3.5e-16, lx 2.2e-16, ly 7.57e-15
#   whole procedure (the counts per million; the planted trend at G = 150 and 400): s 6.55e-15, fit 1.22e-13, ySeq 2.81e-12,
#   weights 5.91e-15, b 5.15e-16, a 3.26e-14, cvDist 1.91e-12, bw 1.08e-15, distMid 1.68e-15, mu 3.97e-15, sigma 1.01e-15,
#   P 1.8e-13;  curve distance alone 6.42e-16;  mode alone (n = 64, 65, 1 000): dens 6.94e-15, bw 4e-16, distMid 7.83e-16
FIG = {"sd": 3.5e-16, "lx": 2.2e-16, "ly": 7.57e-15, "s": 6.55e-15, "fit": 1.22e-13, "ySeq": 2.81e-12, "weights": 5.91e-15, "b": 5.15e-16,
       "a": 3.26e-14, "cvDist": 1.91e-12, "bw": 1.08e-15, "dens": 6.94e-15, "distMid": 1.68e-15, "mu": 3.97e-15, "sigma": 1.01e-15, "P": 1.8e-13}
REL = {k: 8 * v for k, v in FIG.items()}
assert all(v <= (1e-8 if k == "P" else 1e-9) * (1 + 1e-12) for k, v in REL.items())


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(a - b) / np.abs(b)
    d = np.where(a == b, 0.0, d)
    return float(np.nanmax(d)) if np.isfinite(d).any() else 0.0


def same(a, b):
    """The same bits, NaN where the other has NaN."""
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def held(what, **pairs):
    """Prints the largest relative difference of every named (got, want) pair, then holds each to REL."""
    fig = {k: rel(*v) for k, v in pairs.items()}
    print(what, {k: f"{v:.3g}" for k, v in fig.items()})
    assert all(fig[k] <= REL[k] for k in fig), fig


def dev_ops():
    import torch

    ops = gficf_amd.HipOps(0)
    dev = torch.device("cuda", 0)
    return torch, ops, dev, lambda v, dt=np.float64: torch.from_numpy(np.ascontiguousarray(v, dtype=dt)).to(dev)


# ------------------------------------------------------------------ moments
@functools.lru_cache(maxsize=None)
def moment_matrix():
    rng = np.random.default_rng(5)
    X = rng.poisson(0.6, (67, 193)).astype(np.float64) * (rng.random((67, 193)) < .5)
    X[0] = 0                                                              # an empty gene
    X[1] = 0
    X[1, 100] = 4                                                         # one entry
    X[2] = 3                                                              # stored in every cell, constant: sd = 0, invalid
    X[3] = 1 + rng.poisson(2.0, 193)                                      # stored in every cell, varying
    X[4] = 0
    X[4, rng.choice(193, 65, replace=False)] = 1 + rng.poisson(1.0, 65)   # one entry past a wave
    return X, hvg_np.moments(X)


@pytest.mark.parametrize("ptr", [np.int32, np.int64])
def test_moments(ptr):
    X, want = moment_matrix()
    assert list(want["nobs"][:5]) == [0, 1, 193, 193, 65] and list(want["valid"][:5]) == [False, True, False, True, True]
    M = sp.csc_matrix(X)
    M.indptr = M.indptr.astype(ptr)
    got = gficf_amd.gene_moments(M)
    assert np.array_equal(got["mean"], want["mean"]) and np.array_equal(got["nobs"], want["nobs"]) and np.array_equal(got["valid"], want["valid"])
    assert got["sd"][2] == 0 and got["sd"][0] == 0 and np.isnan(got["ly"][0]) and got["ly"][2] == -np.inf
    ok = want["valid"]
    held(f"moments {ptr.__name__}", sd=(got["sd"], want["sd"]), lx=(got["lx"][ok], want["lx"][ok]), ly=(got["ly"][ok], want["ly"][ok]))
    assert rel(got["var"], want["var"]) <= 2 * REL["sd"] + 1e-15


# ------------------------------------------------------------------ the local fit
def fit_case(n, k, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 4, n)
    x[1], x[7] = x[0], x[6]                                               # pairs of equal x
    y = 2.0 + np.sin(1.3 * x) + 0.05 * rng.standard_normal(n)
    grid = np.linspace(x.min(), x.max(), 37)                              # off the data, both ends included
    assert int(np.floor((k / n) * n)) == k
    return x, y, grid


@pytest.mark.parametrize("n,k", [(20, 4), (100, 20), (320, 64), (325, 65), (400, 80)])
def test_local_fit_at_the_data_and_off_it(n, k):
    x, y, grid = fit_case(n, k, n)
    res = y - y.mean()
    w = hvg_np.bisquare(res, np.quantile(np.abs(res), .7) / 6)            # bisquare weights, three in ten of them zero
    assert (w == 0).any() and (w > 0).sum() > n // 2
    for name, wt in (("ones", None), ("bisquare", w)):
        for at_name, at in (("data", None), ("grid", grid)):
            got, h = gficf_amd.local_regression(x, y, at=at, nn=k / n, weights=wt, ret_h=True)
            want, hw = hvg_np.local_fit(x, y, x if at is None else at, k, wt, ret_h=True)
            assert np.array_equal(h, hw), (name, at_name)                 # one subtraction of inputs
            assert same(got, want), (name, at_name, rel(got, want))       # the oracle adds in the kernel's order


def test_local_fit_ties_and_empty_windows():
    n, k = 100, 20
    x, y, grid = fit_case(n, k, 77)
    o = np.argsort(x, kind="stable")
    x[o[60:60 + k + 1]] = x[o[60]]                                        # a run of k + 1 equal x: h = 0 there
    at = np.concatenate([grid, [x[o[60]], x.min()]])
    w = np.ones(n)
    w[np.argsort(x, kind="stable")[:2 * k + 1]] = 0                       # every point near the left end weighs nothing
    got, h = gficf_amd.local_regression(x, y, at=at, nn=k / n, weights=w, ret_h=True)
    want, hw = hvg_np.local_fit(x, y, at, k, w, ret_h=True)
    assert np.array_equal(h, hw) and h[-2] == 0 and np.isnan(want[-1]) and np.isfinite(want[-2])
    assert want[-2] == pytest.approx(y[x == x[o[60]]].mean(), rel=1e-13)
    assert same(got, want), rel(got, want)


def test_robust_loop():
    torch, ops, dev, t = dev_ops()
    n, k = 400, 80
    mean, cv, _ = hvg_np.planted(n, 1)
    o = np.argsort(np.log10(mean), kind="stable")
    xs, ys = np.log10(mean)[o], np.log10(cv)[o]
    ws = torch.empty(ops.hvg_workspace_bytes(n), dtype=torch.uint8, device=dev)
    w, fit, s = (torch.empty(m, dtype=torch.float64, device=dev) for m in (n, n, 3))
    ops.hvg_robust(t(xs), t(ys), k, 3, ws, w, fit, s)
    ops.hvg_sync(ws)
    fw, ww, sw = hvg_np.robust_fit(xs, ys, k)
    assert (ww == 0).any() and (sw > 0).all()
    assert same(s.cpu().numpy(), sw) and same(w.cpu().numpy(), ww) and same(fit.cpu().numpy(), fw)
    with pytest.raises(gficf_amd.GficfError, match="ascending"):
        ops.hvg_robust(t(xs[::-1]), t(ys), k, 3, ws, w, fit, s)
        ops.hvg_sync(ws)


def test_gap_counts():
    torch, ops, dev, t = dev_ops()
    xs = np.sort(np.random.default_rng(3).normal(2.0, 0.7, 100))
    xs[10] = xs[9]
    grid_w = hvg_np.seq(xs[0], xs[-1], 0.005)
    ws = torch.empty(ops.hvg_workspace_bytes(100), dtype=torch.uint8, device=dev)
    grid, gap = torch.empty(len(grid_w), dtype=torch.float64, device=dev), torch.empty(len(grid_w), dtype=torch.int32, device=dev)
    ops.hvg_gap(t(xs), xs[0], 0.005, 0.05, ws, grid, gap)
    ops.hvg_sync(ws)
    want = hvg_np.gap_counts(xs, grid_w)
    assert np.array_equal(grid.cpu().numpy(), grid_w) and np.array_equal(gap.cpu().numpy(), want) and want.max() > 5 and want.min() <= 1


# ------------------------------------------------------------------ distances and the mode
def test_curve_distance():
    rng = np.random.default_rng(11)
    b, a = 50.0, 0.05
    lx = rng.uniform(0, 4, 50)
    lx[0], lx[1] = 0.0, 4.0                                               # clipped windows at both ends
    lx[2] = 0.0 + 1234 * 0.001                                            # exactly on a grid point
    lx[3], lx[4] = (0.0 + 2000 * 0.001) - 0.0001, (0.0 + 3000 * 0.001) + 0.0001      # a hair beside a grid point
    off = rng.choice([-1, 1], 50) * rng.uniform(0.01, 0.3, 50)
    off[3], off[4] = 0.0002, -0.0002                                      # just above with the nearest point to the right; just below, to the left
    ly = hvg_np.curve(10.0 ** lx, b, a) + off
    want, index, sign, margin = hvg_np.curve_distance(lx, ly, b, a, ret_all=True)
    g1 = hvg_np.seq(0.0, 4.0, 0.001)
    yf = hvg_np.curve(10.0 ** g1, b, a)
    right, above = g1[index] > lx, yf[index] < ly
    assert margin.min() > 1e-9 and g1[1234] == lx[2]
    assert all((right == r)[above == u].any() for r in (True, False) for u in (True, False))      # the four branches
    assert (sign[right] == -1).all() and np.array_equal(sign[~right] > 0, above[~right])
    got, gi = gficf_amd.curve_distance(lx, ly, b, a, ret_index=True)
    assert np.array_equal(gi, index) and np.array_equal(np.sign(got), sign)
    held("curve distance", cvDist=(got, want))


@pytest.mark.parametrize("n", [64, 65, 1000])
def test_kde(n):
    torch, ops, dev, t = dev_ops()
    rng = np.random.default_rng(n)
    v = np.where(rng.random(n) < .8, rng.normal(0.1, 0.2, n), rng.normal(1.5, 0.5, n))
    bw, grid, dens = hvg_np.density(v)
    top = np.sort(dens)[-2:]
    assert (top[1] - top[0]) / top[1] > 1e-9
    ws = torch.empty(ops.hvg_workspace_bytes(n), dtype=torch.uint8, device=dev)
    stats, d, am = torch.empty(8, dtype=torch.float64, device=dev), torch.empty(512, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    ops.hvg_kde(t(v), ws, stats, d, am)
    ops.hvg_sync(ws)
    stats = stats.cpu().numpy()
    assert int(am.item()) == int(np.argmax(dens))
    held(f"kde n={n}", bw=(stats[0], bw), dens=(d.cpu().numpy(), dens), distMid=(stats[1], grid[int(np.argmax(dens))]))


# ------------------------------------------------------------------ the whole procedure
@functools.lru_cache(maxsize=None)
def cpm_counts():
    colptr, rowidx, x = synth.counts_csc(2000, 300, 0.07)
    X = gficf_amd.cpm(sp.csc_matrix((x, rowidx, colptr), shape=(2000, 300))).tocsr()
    X = sp.csc_matrix(X[np.diff(X.indptr) > 0])                           # the rows findClusterMarkers leaves
    return X, hvg_np.find_var_genes(X.toarray())


def compare_stages(what, got, want):
    for k in ("n", "k", "cdx0", "j0", "nls_iter"):
        assert got[k] == want[k], k
    assert np.array_equal(got["valid"], want["valid"]) and np.array_equal(got["gap"], want["gap"])
    assert len(got["g5"]) == len(want["g5"]) and np.abs(got["g5"] - want["g5"]).max() <= 1e-14      # the grid starts at min lx, a log10
    assert np.array_equal(gficf_amd.hvg_rows(got["FDR"]), hvg_np.select_rows(want["FDR"]))
    big = want["P"] >= 1e-300
    # from the device's lx and ly, a last bit off NumPy's, the local fit is no longer the oracle's bit for bit.  The weights
    # lie in [0, 1] and end at 0: their difference is taken absolutely (1 + w has it as its relative difference)
    held(what, **{k: (got[k], want[k]) for k in ("s", "fit", "ySeq", "b", "a", "cvDist", "bw", "distMid", "mu", "sigma")},
         weights=(1 + got["weights"], 1 + want["weights"]), P=(got["P"][big], want["P"][big]))
    assert rel(got["FDR"][big], want["FDR"][big]) <= REL["P"]


def test_whole_procedure_on_counts():
    X, want = cpm_counts()
    assert want["cdx0"] > 0 and want["j0"] <= len(want["g5"]) - 2 and want["nls_iter"] > 3
    got = gficf_amd.findVarGenes(X, ret_stages=True)
    assert np.array_equal(got["nobs"], want["nobs"])
    held("counts moments", sd=(got["sd"], want["sd"]), lx=(got["lx"], want["lx"]), ly=(got["ly"], want["ly"]))
    compare_stages("counts_csc(2000, 300, 0.07) as cpm", got, want)
    again = gficf_amd.findVarGenes(X, ret_stages=True)                    # the same bits on every call
    assert set(again) == set(got)
    for k in got:
        assert np.array_equal(np.asarray(got[k]), np.asarray(again[k]), equal_nan=np.asarray(got[k]).dtype.kind == "f"), k
    df = gficf_amd.findVarGenes(X, verbose=False)
    assert list(df.columns) == ["gene", "mean", "cv", "P", "FDR"] and len(df) == X.shape[0]
    assert np.array_equal(df["P"].to_numpy(), got["P"], equal_nan=True) and np.array_equal(df["FDR"].to_numpy(), got["FDR"], equal_nan=True)


@pytest.mark.parametrize("G,seed", [(150, 2), (400, 1)])
def test_whole_procedure_on_a_planted_trend(G, seed):
    mean, cv, up = hvg_np.planted(G, seed)
    mean[3], cv[5] = 0.0, np.nan                                          # two invalid genes
    up = up[(up != 3) & (up != 5)]
    want = hvg_np.var_genes_from_moments(mean, cv)
    got = gficf_amd.var_genes_from_moments(mean, cv)
    assert got["n"] == G - 2 and np.isnan(got["P"][[3, 5]]).all() and np.isnan(got["FDR"][[3, 5]]).all()
    compare_stages(f"planted trend G={G}", got, want)
    assert abs(got["b"] / 50 - 1) < .1 and abs(got["a"] / .05 - 1) < .1 and (got["P"][up] < .05).all()


def test_errors_leave_the_context_usable():
    colptr, rowidx, x = synth.counts_csc(600, 120, 0.07, seed=3)          # one grid point in the trusted range (tests/test_hvg_cpu.py)
    X = gficf_amd.cpm(sp.csc_matrix((x, rowidx, colptr), shape=(600, 120)))
    with pytest.raises(gficf_amd.GficfError, match="the variance-mean trend cannot be fitted"):
        gficf_amd.findVarGenes(X, verbose=False)
    B = X.copy()
    B.indices = B.indices.copy()
    B.indices[-1] = 600
    with pytest.raises(gficf_amd.GficfError, match="GFICF_ERR_BAD_CSC"):
        gficf_amd.gene_moments(B)
    want = hvg_np.moments(X.toarray())
    got = gficf_amd.gene_moments(X)
    assert np.array_equal(got["nobs"], want["nobs"]) and np.array_equal(got["valid"], want["valid"]) and not want["valid"].all()


def test_find_cluster_markers_selects_its_genes_with_locfit():
    X, _ = cpm_counts()
    D = X.toarray()
    D[:60, :100] *= 3.0                                                   # markers of the first cluster
    X = sp.csc_matrix(D)
    data = {"rawCounts": X, "community": np.repeat(["a", "b", "c"], 100), "genes": np.array([f"g{i}" for i in range(X.shape[0])])}
    rows = gficf_amd.hvg_rows(gficf_amd.findVarGenes(X, verbose=False)["FDR"].to_numpy())
    assert len(rows) == 1000 and len(np.unique(rows)) == 1000
    a = gficf_amd.findClusterMarkers(dict(data), hvg="locfit", cpms=X, verbose=False)["de.genes"]
    b = gficf_amd.findClusterMarkers(dict(data), hvg=rows, cpms=X, verbose=False)["de.genes"]
    assert len(a) > 0 and a.equals(b)
    c = gficf_amd.findClusterMarkers(dict(data), hvg=False, cpms=X, verbose=False)["de.genes"]
    assert not a.equals(c)
