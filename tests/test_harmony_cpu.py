"""No GPU: the yardstick of libgficf_harmony.so (tests/helpers/harmony_np.py, which tests/test_harmony_gpu.py measures the
library against) checked against answers derived by algebra and against the quality condition; the bounds the GPU tests use
still say something at every case; the header against its loader and the Makefile; the argument checks of the mirror."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gficf_amd
from tests.helpers import harmony_cases as hc
from tests.helpers import harmony_np as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U, C = hc.U, hc.C


# ------------------------------------------------------------------ the port against the algebra
@pytest.mark.parametrize("n", [33, 64, 257])
@pytest.mark.parametrize("lam", [0.5, 1.0, 10.0])
def test_port_two_balanced_batches_one_cluster(n, lam):
    r = np.random.default_rng(n)
    P, delta = r.standard_normal((n, 3)), np.array([2.0, -1.0, 0.5])
    Z = np.vstack([P, P + delta])
    levels = np.repeat([0, 1], n)[None, :]
    Zcorr, W, flat, _ = hp.correct(Z, levels, 2, np.ones((1, 2 * n)), np.full(2, lam))
    tol = 8 * 2.0 ** -52 * np.abs(delta).max() * n
    assert np.abs((Zcorr[n:] - Zcorr[:n]) - delta * lam / (n + lam)).max() <= tol and flat == 0
    w = n * (P.mean(axis=0) - (P + delta).mean(axis=0)) / (2 * (n + lam))
    assert np.abs(W[0, 1] - w).max() <= tol and np.abs(W[0, 2] + w).max() <= tol and (W[0, 0] == 0).all()


def test_port_one_level_changes_nothing():
    r = np.random.default_rng(4)
    Z = 2 * r.standard_normal((600, 10))
    levels = np.zeros((1, 600), dtype=np.int32)
    Zc, _ = hp.normalise(Z)
    R = hp.assign(Zc, levels, 1, Zc[:20], 0.1)[0]
    Zcorr = hp.correct(Z, levels, 1, R, np.ones(1))[0]
    ratio = np.abs(Zcorr - Z).max() / (4 * 600 * 2.0 ** -52 * np.abs(Z).max())
    print("B = 1: max |Zcorr - Z|", np.abs(Zcorr - Z).max(), "over the bound", ratio)
    assert ratio <= 1


@pytest.mark.parametrize("name", list(hc.CASES))
def test_port_round_properties_and_bounds(name):
    c = hc.case(name)
    P = hp.phi(c["levels"], c["B"])
    R0, _, _, Y0 = hp.round_(c["Zc"], c["levels"], c["B"], c["Y"], c["R"], c["O"], c["E"], np.zeros(c["B"]), hc.SIGMA, c["perm"], c["n_blocks"])
    # theta = 0: the assignment of the new centroids (numpy adds the K terms of a block's columns in another order than a whole
    # matrix's: equal up to that sum's rounding here, in bits on the device, where both are one kernel)
    A0 = hp.assign(c["Zc"], c["levels"], c["B"], Y0, hc.SIGMA)[0]
    assert (np.abs(R0 - A0) <= c["K"] * 2.0 ** -52 * A0).all()
    assert np.abs(c["R1"].sum(axis=0) - 1).max() <= c["K"] * 2.0 ** -52 and np.abs(c["R"].sum(axis=0) - 1).max() <= c["K"] * 2.0 ** -52
    n = c["N"] + 2 * c["n_blocks"] + 2
    O, E = c["R1"] @ P.T, np.outer(c["R1"].sum(axis=1), P.mean(axis=1))
    assert (np.abs(c["O1"] - O) <= C * n * U * O).all() and (np.abs(c["E1"] - E) <= C * n * U * E).all()
    # the inputs are separated blobs: no hard assignment is a near tie, every blob has its cluster
    assert (hp.start_margin(c["Zc"], c["Y"]) > 1e-9).all() and len(np.unique(c["lab"])) == c["K"]
    # a level without cells where the case asks for one; the blocks the case is there for
    if c.get("empty"):
        assert (c["levels"] != c["B"] - 1).all() and P[-1].sum() == 0
    sizes = [len(b) for b in np.array_split(c["perm"], c["n_blocks"])]
    assert {"n7": sizes.count(0) == 13, "n61": sorted(set(sizes)) == [3, 4]}.get(name, True)
    # the bounds the GPU tests allow still say something
    dD = float(hc.dist_bound(c["Y1"], c["Zc"]).max()) + hc.centroid_dist_shift(c["R"], c["Zc"])
    assert hc.round_rel_bound(c, dD) < 1e-6 and hc.soft_rel_bound(hc.dist_bound(c["Y"], c["Zc"]).max(), hc.SIGMA, c["K"]) < 1e-9
    assert c["flat"] == 0 and C * (c["N"] + (c["B"] + 1) ** 2) * U * c["cond"] < 1e-6


def test_port_empty_cluster_and_zero_row():
    Zc, zero = hp.normalise(np.array([[3.0, 4.0], [0.0, 0.0], [0.0, -2.0]]))
    assert zero == 1 and np.array_equal(Zc, [[0.6, 0.8], [0.0, 0.0], [0.0, -1.0]])
    # the second centroid attracts nothing: it stays; the tie of the zero row goes to the lowest k
    Y, lab = hp.start(Zc[[0, 1]], np.array([[1.0, 0.0], [-1.0, 0.0]]), 2)
    assert np.array_equal(lab, [0, 0]) and np.array_equal(Y[1], [-1.0, 0.0]) and np.allclose(Y[0], [0.6, 0.8])
    # a cluster without mass is left out of the correction and counted
    c = hc.case("v2")
    R = np.array(c["R1"])
    R[3] = 0
    Zcorr, W, flat, _ = hp.correct(c["Z"], c["levels"], c["B"], R, c["lamb_b"])
    assert flat == 1 and (W[3] == 0).all() and np.isfinite(Zcorr).all()


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("hseed", [0, 1])
def test_port_quality(seed, hseed):
    X, ct, b = hp.quality_data(seed)
    cells, perm = gficf_amd.harmony_draws(600, 20, 200, hseed)
    r = hp.harmony(X, b[None, :].astype(np.int32), 3, np.full(3, 2.0), np.full(3, 1.0), 0.1, hp.normalise(X[cells])[0], perm, 10, 10, 20, 20, 1e-5, 1e-4)
    before, after = hp.quality(X, ct, b), hp.quality(r["Z"], ct, b)
    print(f"seed {seed}/{hseed}: type share {before[0]:.4f} -> {after[0]:.4f}, mixing {before[1]:.3f} -> {after[1]:.3f}, {r['iterations']} iterations")
    assert after[0] >= 0.99 and after[1] >= 0.8 and before[1] < 0.1 and r["converged"] and 2 <= r["iterations"] <= 6


# ------------------------------------------------------------------ plumbing
def test_header_and_loader_name_the_same_entries():
    from gficf_amd import _harmony_lib as lib

    text = open(os.path.join(ROOT, "include", "gficf_harmony.h")).read()
    body = text[text.index("extern \"C\""):]
    declared = re.findall(r"\b(gficf_harmony_\w+)\s*\(([^;]*)\)\s*;", body)
    assert set(n for n, _ in declared) == set(lib.SIGNATURES) and len(declared) == 10
    for name, args in declared:
        n = 0 if args.strip() == "void" else args.count(",") + 1
        assert n == len(lib.SIGNATURES[name][1]), name
    assert "#define GFICF_HARMONY_ABI_VERSION 1" in text and lib.ABI_VERSION == 1
    for macro, value in (("MAX_D", lib.MAX_D), ("MAX_K", lib.MAX_K), ("MAX_B", lib.MAX_B), ("MAX_V", lib.MAX_V)):
        assert re.search(rf"#define\s+GFICF_HARMONY_{macro}\s+{value}\b", text), macro
    assert (lib.MAX_D, lib.MAX_K, lib.MAX_B, lib.MAX_V) == (128, 100, 64, 4)
    core = open(os.path.join(ROOT, "include", "gficf_hip.h")).read()
    assert re.search(r"#define\s+GFICF_HIP_ABI_VERSION\s+7\b", core)


def test_makefile_builds_the_library_with_the_others():
    csrc = os.path.join(ROOT, "gficf_amd", "csrc")
    build = subprocess.run(["make", "-n", "-B", "-C", csrc, "all"], capture_output=True, text=True, check=True).stdout.splitlines()
    link = [ln for ln in build if " -o ../libgficf_harmony.so " in ln]
    assert len(link) == 1 and re.search(r"hipcc --offload-arch=gfx950 -shared -fPIC -o \.\./libgficf_harmony\.so harmony\.o -L\.\. -lgficf_hip\b", link[0])
    comp = [ln for ln in build if ln.endswith(" -o harmony.o")]
    assert len(comp) == 1 and "-ffp-contract=off" in comp[0] and "--offload-arch=gfx950" in comp[0] and "fast-math" not in comp[0]
    clean = subprocess.run(["make", "-n", "-C", csrc, "clean"], capture_output=True, text=True, check=True).stdout
    assert re.search(r"^rm -f .*\bharmony\.o\b.* \.\./libgficf_harmony\.so\b", clean, re.M)


def test_loader(monkeypatch):
    from gficf_amd import _harmony_lib as lib

    L = lib.load()
    assert isinstance(L, ctypes.CDLL) and lib.load() is L and L.gficf_harmony_abi_version() == lib.ABI_VERSION
    for sym, (res, args) in lib.SIGNATURES.items():
        fn = getattr(L, sym)
        assert fn.restype is res and list(fn.argtypes) == list(args), sym
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert sorted(set(re.findall(r" T (gficf_[a-z0-9_]+)$", out, re.M))) == sorted(lib.SIGNATURES)
    wb = L.gficf_harmony_workspace_bytes
    assert wb(600, 10, 20, 1, 3) >= 8 * 20 * 600 and wb(600, 10, 20, 2, 6) > wb(600, 10, 20, 1, 6) and wb(54000, 50, 100, 1, 4) < 100 << 20
    for bad in ((0, 10, 1, 1, 1), (600, 0, 20, 1, 3), (600, 129, 20, 1, 3), (600, 10, 101, 1, 3), (600, 10, 0, 1, 3), (10, 10, 11, 1, 3), (600, 10, 20, 5, 8),
                (600, 10, 20, 0, 3), (600, 10, 20, 1, 65), (600, 10, 20, 3, 2), (2 ** 31, 10, 20, 1, 3)):
        assert wb(*bad) == 0, bad
    assert wb(600, 128, 100, 4, 64) > 0
    monkeypatch.setattr(lib, "LIB_PATH", os.path.join(os.path.dirname(lib.LIB_PATH), "libgficf_harmony_missing.so"))
    with pytest.raises(ImportError, match="not found: build it with"):
        lib.load()


def test_surface():
    p = inspect.signature(gficf_amd.runHarmony).parameters
    want = dict(theta=2.0, lamb=1.0, sigma=0.1, nclust=None, tau=0.0, block_size=0.05, max_iter_harmony=10, max_iter_kmeans=20, epsilon_cluster=1e-5,
                epsilon_harmony=1e-4, seed=180582)
    assert list(p)[:2] == ["data", "batch"] and {k: p[k].default for k in want} == want
    q = inspect.signature(gficf_amd.harmony_matrix).parameters
    assert list(q)[:2] == ["X", "batch"] and {k: q[k].default for k in want} == want
    for name in ("harmony_start", "harmony_assign", "harmony_round", "harmony_objective", "harmony_correct", "harmony_normalise"):
        assert callable(getattr(gficf_amd, name)) and callable(getattr(gficf_amd.HipOps, name)), name
    assert callable(gficf_amd.HipOps.harmony) and callable(gficf_amd.HipOps.harmony_sync) and callable(gficf_amd.HipOps.harmony_workspace_bytes)


def test_levels_and_draws():
    lev, vs, names, labels = gficf_amd.harmony_levels(np.array(["b", "a", "b", "c"]), 4)
    assert np.array_equal(lev, [[0, 1, 0, 2]]) and lev.dtype == np.int32 and np.array_equal(vs, [0, 3]) and names == ["batch"] and list(labels[0]) == ["b", "a", "c"]
    lev, vs, names, labels = gficf_amd.harmony_levels({"run": [5, 5, 3, 3], "donor": ["x", "y", "x", "y"]}, 4)
    assert np.array_equal(lev, [[0, 0, 1, 1], [2, 3, 2, 3]]) and np.array_equal(vs, [0, 2, 4]) and names == ["run", "donor"]
    import pandas as pd

    assert np.array_equal(gficf_amd.harmony_levels(pd.DataFrame({"run": [5, 5, 3, 3], "donor": ["x", "y", "x", "y"]}), 4)[0], lev)
    cells, perm = gficf_amd.harmony_draws(50, 7, 3, 11)
    r = np.random.default_rng(11)
    assert np.array_equal(cells, r.choice(50, 7, replace=False)) and len(set(cells)) == 7 and perm.dtype == np.int32 and perm.shape == (3, 50)
    assert all(np.array_equal(perm[i], r.permutation(50)) for i in range(3))
    assert np.array_equal(gficf_amd.harmony_draws(50, 7, 5, 11)[1][:3], perm)            # a longer run draws the same first rounds


def test_argument_checks():
    """Everything the mirror refuses, it refuses before it touches a device."""
    X, b = np.random.default_rng(0).standard_normal((40, 3)), np.arange(40) % 2
    hm = gficf_amd.harmony_matrix
    for kw, msg in ((dict(sigma=0.0), "sigma"), (dict(sigma=np.inf), "sigma"), (dict(block_size=0.0), "block_size"), (dict(block_size=1.5), "block_size"),
                    (dict(theta=-1.0), "theta"), (dict(lamb=-1.0), "lamb"), (dict(theta=[1.0, 2.0, 3.0]), "theta"), (dict(nclust=0), "clusters"),
                    (dict(nclust=41), "clusters"), (dict(nclust=101), "clusters"), (dict(tau=-1.0), "tau"), (dict(max_iter_harmony=-1), "limits")):
        with pytest.raises(ValueError, match=msg):
            hm(X, b, **kw)
    with pytest.raises(ValueError, match="one label per cell"):
        hm(X, b[:-1])
    with pytest.raises(ValueError, match="at most 64"):
        hm(np.zeros((130, 2)) + 1, np.arange(130) % 65)
    with pytest.raises(ValueError, match="1 to 4 variables"):
        hm(X, {str(i): b for i in range(5)})
    with pytest.raises(ValueError, match="1 <= d <= 128"):
        hm(np.ones((40, 129)), b)
    with pytest.raises(ValueError, match="not finite"):
        hm(np.where(np.arange(120).reshape(40, 3) == 5, np.nan, X), b)
    with pytest.raises(ValueError, match="First run runPCA"):
        gficf_amd.runHarmony({}, b)
    with pytest.raises(ValueError, match="outside its variable"):
        gficf_amd.harmony_assign(X, np.full((1, 40), 2, dtype=np.int32), [0, 2], X[:2], 0.1)
    with pytest.raises(ValueError, match="var_start"):
        gficf_amd.harmony_assign(X, np.zeros((1, 40), dtype=np.int32), [0, 0], X[:2], 0.1)
    with pytest.raises(ValueError, match="permutation"):
        gficf_amd.harmony_round(X, b[None, :], [0, 2], X[:2], np.ones((2, 40)) / 2, np.ones((2, 2)), np.ones((2, 2)), 2.0, 0.1, np.zeros(40), 5)
    with pytest.raises(ValueError, match="K x N"):
        gficf_amd.harmony_correct(X, b[None, :], [0, 2], np.ones((2, 39)))
    with pytest.raises(ValueError, match="Y0 must be K x d"):
        gficf_amd.harmony_start(X, np.ones((2, 4)))


def test_new_cells_are_refused_after_harmony():
    data = {"pca": {"cells": np.zeros((4, 2)), "harmony": {"iterations": 3}}, "uwot": {"space": "pca"}, "genes": np.arange(3), "w": np.ones(3)}
    with pytest.raises(NotImplementedError, match="embedNewCells after runHarmony.*not batch corrected"):
        gficf_amd.embedNewCells(data, None, verbose=False)
    import pandas as pd

    data["embedded"] = pd.DataFrame({"X": [0.0, 1.0], "Y": [0.0, 1.0], "predicted": ["NO", "YES"]})
    with pytest.raises(NotImplementedError, match="classify_cells.*after runHarmony"):
        gficf_amd.classify_cells(data, ["a"], method="PCA")
