"""Harmony on the device (include/gficf_harmony.h, libgficf_harmony.so): the answers derived by algebra, every stage against the
NumPy port from the port's own state within bounds formed from the port's absolute sums (tests/helpers/harmony_cases.py), the
chain against its stages bit for bit, the quality condition, and the runHarmony mirror."""
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gficf_amd  # noqa: E402
from tests.helpers import harmony_cases as hc  # noqa: E402
from tests.helpers import harmony_np as hp  # noqa: E402

pytestmark = pytest.mark.gpu
U, C = hc.U, hc.C
NAMES = list(hc.CASES)


def ratio(got, want, bound, what):
    """max |got - want| / bound, printed before it is asserted below 1."""
    err = np.abs(np.asarray(got) - np.asarray(want))
    r = float(np.max(err / bound)) if err.size else 0.0
    print(f"{what}: max err {float(err.max()) if err.size else 0.0:.3g}, err / bound {r:.3g}")
    return r


# ------------------------------------------------------------------ derived answers
@pytest.mark.parametrize("n", [33, 64, 257])
@pytest.mark.parametrize("lam", [0.5, 1.0, 10.0])
def test_two_balanced_batches_one_cluster(n, lam):
    """R = 1: the normal equations solve to w1 = -w2 = n (m1 - m2) / (2 (n + lam)), the batch gap becomes delta lam / (n + lam)."""
    r = np.random.default_rng(n)
    P, delta = r.standard_normal((n, 3)), np.array([2.0, -1.0, 0.5])
    Z = np.vstack([P, P + delta])
    levels = np.repeat([0, 1], n)[None, :].astype(np.int32)
    got = gficf_amd.harmony_correct(Z, levels, [0, 2], np.ones((1, 2 * n)), lam)
    tol = 8 * 2.0 ** -52 * np.abs(delta).max() * n
    gap = got["Z"][n:] - got["Z"][:n]
    print("gap err / tol", np.abs(gap - delta * lam / (n + lam)).max() / tol)
    assert np.abs(gap - delta * lam / (n + lam)).max() <= tol and got["flat_clusters"] == 0
    w = n * (P.mean(axis=0) - (P + delta).mean(axis=0)) / (2 * (n + lam))
    assert np.abs(got["W"][0, 1] - w).max() <= tol and np.abs(got["W"][0, 2] + w).max() <= tol and (got["W"][0, 0] == 0).all()


def test_one_level_changes_nothing():
    """B = 1: the intercept takes everything, Zcorr = Z up to rounding: 4 N 2^-52 max |Z|."""
    r = np.random.default_rng(4)
    Z = 2 * r.standard_normal((600, 10))
    levels, vs = np.zeros((1, 600), dtype=np.int32), [0, 1]
    Zc = gficf_amd.harmony_normalise(Z)
    R = gficf_amd.harmony_assign(Zc, levels, vs, Zc[:20], 0.1)["R"]
    got = gficf_amd.harmony_correct(Z, levels, vs, R, 1.0)
    bound = 4 * 600 * 2.0 ** -52 * np.abs(Z).max()
    assert ratio(got["Z"], Z, bound, "B = 1, Zcorr against Z") <= 1 and got["flat_clusters"] == 0


@pytest.mark.parametrize("name", NAMES)
def test_round_properties(name):
    """theta = 0: the round is the assignment of its new centroids, in bits; the columns of R sum to 1; O and E are R Phi^T and
    (sum R) Pr recomputed, after every one of three rounds."""
    c = hc.case(name)
    Phi = hp.phi(c["levels"], c["B"])
    z = gficf_amd.harmony_round(c["Zc"], c["levels"], c["var_start"], c["Y"], c["R"], c["O"], c["E"], 0.0, hc.SIGMA, c["perm"], c["n_blocks"])
    a = gficf_amd.harmony_assign(c["Zc"], c["levels"], c["var_start"], z["Y"], hc.SIGMA)
    assert np.array_equal(z["R"], a["R"])
    st = {k: c[k] for k in ("R", "O", "E", "Y")}
    for rnd in range(1, 4):
        perm = np.random.default_rng(rnd).permutation(c["N"]).astype(np.int32)
        st = gficf_amd.harmony_round(c["Zc"], c["levels"], c["var_start"], st["Y"], st["R"], st["O"], st["E"], c["theta_b"], hc.SIGMA, perm, c["n_blocks"])
        assert np.isfinite(st["R"]).all() and np.abs(st["R"].sum(axis=0) - 1).max() <= c["K"] * 2.0 ** -52
        O, S = st["R"] @ Phi.T, st["R"].sum(axis=1)
        n = c["N"] + 2 * c["n_blocks"] * rnd + 2
        assert ratio(st["O"], O, C * n * U * O + 1e-300, f"{name} round {rnd} O") <= 1
        assert ratio(st["E"], np.outer(S, Phi.mean(axis=1)), C * n * U * np.outer(S, Phi.mean(axis=1)) + 1e-300, f"{name} round {rnd} E") <= 1


# ------------------------------------------------------------------ the stages against the port
@pytest.mark.parametrize("name", NAMES)
def test_normalise_and_start(name):
    c = hc.case(name)
    Zc = gficf_amd.harmony_normalise(c["Z"])
    assert ratio(Zc, c["Zc"], C * (c["d"] + 2) * U, f"{name} Zc") <= 1
    got = gficf_amd.harmony_start(c["Zc"], c["Y0"], hc.INIT_ITER)
    # the hard assignments: exact wherever the port's two best dot products are 1e-9 apart; at most 1 % of the cells left out
    clear = hp.start_margin(c["Zc"], c["Y"]) > 1e-9
    assert clear.mean() >= 0.99 and np.array_equal(got["labels"][clear], c["lab"][clear])
    if clear.all():
        onehot = (c["lab"][None, :] == np.arange(c["K"])[:, None]).astype(np.float64)
        assert ratio(got["Y"], c["Y"], hc.centroid_bound(onehot, c["Zc"]) + 1e-300, f"{name} start Y") <= 1
    same = gficf_amd.harmony_start(c["Zc"], c["Y0"], 0)
    assert np.array_equal(same["Y"], c["Y0"]) and (same["labels"] == 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_assign(name):
    c = hc.case(name)
    got = gficf_amd.harmony_assign(c["Zc"], c["levels"], c["var_start"], c["Y"], hc.SIGMA)
    eR = hc.soft_rel_bound(hc.dist_bound(c["Y"], c["Zc"]).max(axis=0), hc.SIGMA, c["K"])          # per cell
    assert ratio(got["R"], c["R"], eR[None, :] * c["R"] + 1e-300, f"{name} assign R") <= 1
    rel = C * c["N"] * U + eR.max()
    assert ratio(got["O"], c["O"], rel * c["O"] + 1e-300, f"{name} assign O") <= 1
    assert ratio(got["E"], c["E"], (rel + C * 4 * U) * c["E"] + 1e-300, f"{name} assign E") <= 1


@pytest.mark.parametrize("name", NAMES)
def test_round_objective_correct(name):
    c = hc.case(name)
    got = gficf_amd.harmony_round(c["Zc"], c["levels"], c["var_start"], c["Y"], c["R"], c["O"], c["E"], c["theta_b"], hc.SIGMA, c["perm"], c["n_blocks"])
    bY = hc.centroid_bound(c["R"], c["Zc"])
    assert ratio(got["Y"], c["Y1"], bY + 1e-300, f"{name} round Y") <= 1
    dD = float(hc.dist_bound(c["Y1"], c["Zc"]).max()) + hc.centroid_dist_shift(c["R"], c["Zc"])   # dist moves with the centroids
    eR = hc.round_rel_bound(c, dD)
    print(f"{name}: relative bound of R after the round {eR:.3g}")
    assert eR < 1e-6                                           # the bound still says something
    assert ratio(got["R"], c["R1"], eR * c["R1"] + 1e-300, f"{name} round R") <= 1
    rel = C * (c["N"] + 2 * c["n_blocks"]) * U + eR
    assert ratio(got["O"], c["O1"], rel * c["O1"] + 1e-300, f"{name} round O") <= 1
    assert ratio(got["E"], c["E1"], (rel + C * 4 * U) * c["E1"] + 1e-300, f"{name} round E") <= 1
    # the objective from the port's state: K N terms in another order, and dist recomputed
    terms = hp.objective_terms(c["Zc"], c["levels"], c["B"], c["Y1"], c["R1"], c["O1"], c["E1"], c["theta_b"], hc.SIGMA)
    absum = sum(np.abs(t).sum() for t in terms)
    obj = gficf_amd.harmony_objective(c["Zc"], c["levels"], c["var_start"], c["Y1"], c["R1"], c["O1"], c["E1"], c["theta_b"], hc.SIGMA)
    bound = C * c["K"] * c["N"] * U * absum + float((c["R1"] * hc.dist_bound(c["Y1"], c["Zc"])).sum()) + C * 8 * U * absum
    assert ratio(obj, c["obj"], bound, f"{name} objective") <= 1
    # the correction from the port's R: the moments are sums of N terms, the solve multiplies their error by cond(A_k)
    cor = gficf_amd.harmony_correct(c["Z"], c["levels"], c["var_start"], c["R1"], c["lamb_b"])
    n = c["N"] + (c["B"] + 1) ** 2
    bound = C * n * U * c["cond"] * c["V"] * (np.abs(c["W"]).max() + np.abs(c["Z"]).max()) + C * c["K"] * U * np.abs(c["Z"]).max()
    assert cor["flat_clusters"] == c["flat"] == 0
    assert ratio(cor["Z"], c["Zcorr"], bound, f"{name} Zcorr (cond {c['cond']:.3g})") <= 1
    assert ratio(cor["W"], c["W"], bound, f"{name} W") <= 1


def test_cluster_without_mass_contributes_nothing():
    """A row of R that is zero: its pivot is not positive, it is counted and left out; nothing is NaN."""
    c = hc.case("v2")
    R = np.array(c["R1"])
    R[3] = 0.0
    got = gficf_amd.harmony_correct(c["Z"], c["levels"], c["var_start"], R, c["lamb_b"])
    want = hp.correct(c["Z"], c["levels"], c["B"], R, c["lamb_b"])
    assert got["flat_clusters"] == want[2] == 1 and np.isfinite(got["Z"]).all() and (got["W"][3] == 0).all()
    assert np.abs(got["Z"] - want[0]).max() < 1e-9


def test_deferred_errors():
    c = hc.case("n7")
    from gficf_amd.api import _harmony_ops
    import torch

    ops, dev = _harmony_ops(0), "cuda:0"
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)  # noqa: E731
    ws = torch.zeros(ops.harmony_workspace_bytes(7, 2, 2, 1, 2), dtype=torch.uint8, device=dev)
    R, O, E, Y = t(c["R"]), t(c["O"]), t(c["E"]), t(c["Y"])
    bad = np.array(c["perm"])
    bad[2] = 7
    ops.harmony_round(t(c["Zc"]), t(c["levels"]), c["var_start"], t(c["theta_b"]), 0.1, t(bad), 20, R, O, E, Y, ws)
    with pytest.raises(gficf_amd.GficfError, match="perm"):
        ops.harmony_sync(ws)
    ws.zero_()
    lev = np.array(c["levels"])
    lev[0, 0] = 2
    ops.harmony_assign(t(c["Zc"]), t(lev), c["var_start"], Y, 0.1, R, O, E, ws)
    with pytest.raises(gficf_amd.GficfError, match="level"):
        ops.harmony_sync(ws)
    with pytest.raises(gficf_amd.GficfError):
        ops.harmony_assign(t(c["Zc"]), t(c["levels"]), c["var_start"], Y, 0.0, R, O, E, ws)


# ------------------------------------------------------------------ the chain
def composed(X, batch, max_iter_harmony, max_iter_kmeans=20, **kw):
    """The chain of include/gficf_harmony.h out of the stage entries, device-resident, with harmony_matrix's own inputs."""
    import torch
    from gficf_amd import api

    p = api._harmony_setup(X, batch, kw.get("theta", 2.0), kw.get("lamb", 1.0), 0.1, kw.get("nclust"), 0.0, 0.05, max_iter_harmony, max_iter_kmeans, 1e-5, 1e-4,
                           10)
    s = api._HarmonyState(p["X"], p["levels"], p["var_start"], p["K"])
    ops, K, vs = s.ops, p["K"], p["var_start"]
    cells, perm = gficf_amd.harmony_draws(s.N, K, max_iter_harmony * max_iter_kmeans, kw.get("seed", 180582))
    Y = s.up(p["X"][cells])
    ops.harmony_normalise(Y, Y, s.ws)
    Zc, Zcorr, R, O, E = s.f64(s.N, s.d), s.Z.clone(), s.f64(K, s.N), s.f64(K, s.B), s.f64(K, s.B)
    lab, obj, theta, lamb, permd = torch.zeros(s.N, dtype=torch.int32, device=s.dev), s.f64(1), s.up(p["theta"]), s.up(p["lamb"]), s.up(perm)
    ops.harmony_normalise(s.Z, Zc, s.ws)
    ops.harmony_start(Zc, Y, 10, Y, lab, s.ws)
    ops.harmony_assign(Zc, s.levels, vs, Y, 0.1, R, O, E, s.ws)

    def objective():
        ops.harmony_objective(Zc, s.levels, vs, Y, R, O, E, theta, 0.1, obj, s.ws)
        return float(obj.cpu()[0])

    objs, used, rounds, h, converged = [objective()], 0, [], [], False
    for it in range(1, max_iter_harmony + 1):
        t = 0
        while t < max_iter_kmeans:
            ops.harmony_round(Zc, s.levels, vs, theta, 0.1, permd[used], p["n_blocks"], R, O, E, Y, s.ws)
            used, t = used + 1, t + 1
            objs.append(objective())
            if t >= 3 and (sum(objs[-4:-1]) - sum(objs[-3:])) / abs(sum(objs[-4:-1])) < 1e-5:
                break
        rounds.append(t)
        ops.harmony_correct(s.Z, s.levels, vs, R, lamb, Zcorr, s.ws)
        ops.harmony_normalise(Zcorr, Zc, s.ws)
        h.append(objs[-1])
        if it >= 2 and (h[-2] - h[-1]) / abs(h[-2]) < 1e-4:
            converged = True
            break
    s.sync()
    return {"Z": Zcorr.cpu().numpy(), "R": R.cpu().numpy(), "Y": Y.cpu().numpy(), "objective_rounds": np.array(objs), "iter_rounds": np.array(rounds),
            "converged": converged}


@pytest.fixture(scope="module")
def quality_runs():
    out = {}
    for seed in (1, 2, 3):
        X, ct, b = hp.quality_data(seed)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            out[seed] = (X, ct, b, gficf_amd.harmony_matrix(X, b, seed=0))
    return out


def test_chain_is_its_stages_and_repeats(quality_runs):
    X, ct, b, r = quality_runs[1]
    again = gficf_amd.harmony_matrix(X, b, seed=0)
    parts = composed(X, b, 10, seed=0)
    for k in ("Z", "R", "Y", "objective_rounds", "iter_rounds"):
        assert np.array_equal(r[k], again[k]), k
        assert np.array_equal(r[k], parts[k]), k
    assert r["converged"] == parts["converged"] and r["iterations"] == len(parts["iter_rounds"])
    # two variables and a run that the limit stops
    both = {"a": b, "b": ct % 2}
    short, long = gficf_amd.harmony_matrix(X, both, max_iter_harmony=2, seed=3), gficf_amd.harmony_matrix(X, both, max_iter_harmony=4, seed=3)
    parts = composed(X, both, 2, seed=3)
    for k in ("Z", "R", "Y", "objective_rounds", "iter_rounds"):
        assert np.array_equal(short[k], parts[k]), k
    n = short["rounds"]
    assert short["iterations"] == 2 and long["iterations"] >= 2 and np.array_equal(long["iter_rounds"][:2], short["iter_rounds"])
    assert np.array_equal(long["objective_rounds"][:n + 1], short["objective_rounds"])


def test_chain_against_the_port(quality_runs):
    """The whole run next to the port's with the same draws: the same rounds, and corrected cells that agree far inside the
    spread of the data (errors grow through the rounds: no bound is claimed for a whole run, the stages carry the bounds)."""
    X, ct, b, r = quality_runs[2]
    cells, perm = gficf_amd.harmony_draws(600, 20, 200, 0)
    want = hp.harmony(X, b[None, :].astype(np.int32), 3, np.full(3, 2.0), np.full(3, 1.0), 0.1, hp.normalise(X[cells])[0], perm, 10, 10, 20, 20, 1e-5, 1e-4)
    print("chain against the port: max |dZ|", np.abs(r["Z"] - want["Z"]).max(), "rounds", r["iter_rounds"], want["iter_rounds"])
    assert np.array_equal(r["iter_rounds"], want["iter_rounds"]) and r["converged"] == want["converged"]
    assert np.abs(r["Z"] - want["Z"]).max() < 1e-6 and np.allclose(r["objective"], want["h"], rtol=1e-9)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_quality(quality_runs, seed):
    X, ct, b, r = quality_runs[seed]
    before, after = hp.quality(X, ct, b), hp.quality(r["Z"], ct, b)
    print(f"seed {seed}: type share {before[0]:.4f} -> {after[0]:.4f}, mixing {before[1]:.3f} -> {after[1]:.3f} of the expectation, "
          f"{r['iterations']} iterations, {r['rounds']} rounds")
    assert after[0] >= 0.99 and after[1] >= 0.8 and r["converged"]


# ------------------------------------------------------------------ the mirror
def test_run_harmony_mirror(quality_runs):
    X, ct, b, r = quality_runs[3]
    data = gficf_amd.runHarmony({"pca": {"cells": X.copy()}}, b, seed=0)
    pca = data["pca"]
    assert np.array_equal(pca["cells"], r["Z"]) and np.array_equal(pca["cells_uncorrected"], X)
    assert pca["harmony"]["converged"] and pca["harmony"]["iterations"] == r["iterations"] and np.array_equal(pca["harmony"]["objective"], r["objective"])
    assert pca["harmony"]["nclust"] == 20 and list(pca["harmony"]["levels"]["batch"]) == list(dict.fromkeys(b.tolist()))
    data = gficf_amd.runHarmony(data, b, seed=0)                 # again: from cells_uncorrected, so the same result
    assert np.array_equal(data["pca"]["cells"], r["Z"]) and np.array_equal(data["pca"]["cells_uncorrected"], X)
    with pytest.warns(UserWarning, match=r"did not converge in 2 iterations.*relative change of the objective was \d"):
        gficf_amd.runHarmony({"pca": {"cells": X.copy()}}, b, max_iter_harmony=2, seed=0)
    data = gficf_amd.clustcells(data, k=15, community_algo="leiden", verbose=False, store_graph=False)
    assert len(data["cluster"]) == 600
    data = gficf_amd.runReduction(data, n_epochs=20, verbose=False)
    assert np.asarray(data["embedded"])[:, :2].shape == (600, 2)
    import scipy.sparse as sp

    with pytest.raises(NotImplementedError, match="runHarmony.*not batch corrected"):
        gficf_amd.embedNewCells(data, sp.csc_matrix((5, 3)), verbose=False)
    emb = data["embedded"].copy()
    emb["predicted"] = ["NO"] * 597 + ["YES"] * 3
    with pytest.raises(NotImplementedError, match="runHarmony"):
        gficf_amd.classify_cells(dict(data, embedded=emb), ["x"] * 597, method="PCA")
