"""No GPU: the yardstick of libgficf_nmf.so (tests/helpers/nmf_np.py, which tests/test_nmf_gpu.py measures the library against)
checked against an independent solver and against the optimality conditions; the header against its loader and the Makefile;
the argument checks of the mirror; the dispatch of pca_project."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.optimize
import scipy.sparse as sp

import gficf_amd
from tests.helpers import nmf_cases as nc
from tests.helpers import nmf_np as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the restatement
def lawson_hanson_problems():
    r = np.random.default_rng(3)
    X = r.random((30, 7))
    return X, [r.random(30) - 0.5 * i / 20 for i in range(20)]


def test_restatement_against_scipy_nnls():
    """nnls_cd(X'X, X'y) at cd_tol = 1e-12 against scipy.optimize.nnls(X, y) (Lawson-Hanson, an active-set method): 30 x 7 uniform
    X, 20 right-hand sides that grow more negative, so the later ones have zeros in their solution.  Within 1e-10 absolute."""
    X, ys = lawson_hanson_problems()
    H, sweeps = nn.nnls_cd(X.T @ X, np.array([X.T @ y for y in ys]), cd_tol=1e-12, cd_maxit=100000)
    want = np.array([scipy.optimize.nnls(X, y)[0] for y in ys])
    err = np.abs(H - want).max()
    print("restatement against scipy.optimize.nnls: max abs err", err, "sweeps up to", sweeps.max(), "zeros", int((want == 0).sum()))
    assert err <= 1e-10 and (want == 0).any() and (want > 0).any()


def test_restatement_meets_the_kkt_conditions():
    """h >= 0; the gradient g = S h - b is >= -eps where h = 0 and |g| <= eps where h > 0.  eps: the inner stop leaves every
    coordinate within cd_tol (h + 1e-15) of its line minimum, that is |g_j| <= cd_tol (h_j + 1e-15) S_jj as the sweep saw it,
    and the later steps of the same sweep move g_j by at most sum_l |S_jl| times their own steps: eps = 2 cd_tol max_j (sum_l
    |S_jl|) (max h + 1)."""
    X, ys = lawson_hanson_problems()
    S, B = X.T @ X, np.array([X.T @ y for y in ys])
    cd_tol = 1e-12
    H, _ = nn.nnls_cd(S, B, cd_tol=cd_tol, cd_maxit=100000)
    g = H @ S - B
    eps = 2 * cd_tol * np.abs(S).sum(axis=1).max() * (H.max() + 1)
    print("KKT: min g at h = 0", g[H == 0].min(), "max |g| at h > 0", np.abs(g[H > 0]).max(), "eps", eps)
    assert (H >= 0).all() and (g[H == 0] >= -eps).all() and (np.abs(g[H > 0]) <= eps).all()


@pytest.mark.parametrize("k,M,warm", [(5, 7, True), (5, 7, False), (65, 3, True), (1, 4, False)])
def test_restatement_rows_at_once_equal_row_by_row(k, M, warm):
    S, B, H0 = nc.solve_case(k, M, warm=warm)
    for kw in (dict(), dict(cd_maxit=1), dict(cd_maxit=3), dict(cd_tol=0.0, cd_maxit=7)):
        H, sw = nn.nnls_cd(S, B, H0, **kw)
        for i in range(M):
            h, s = nn.nnls_row(S, B[i], None if H0 is None else H0[i], **kw)
            assert np.array_equal(h, H[i]) and s == sw[i], (kw, i)
    assert (nn.nnls_cd(S, B, H0, cd_tol=0.0, cd_maxit=7)[1] == 7).all()


def test_restatement_edge_rules():
    S, B, _ = nc.solve_case(6, 9)
    H, sw = nn.nnls_cd(S, -np.abs(B) - 1)
    assert (H == 0).all() and (sw == 1).all()                  # nothing moves: one sweep, exactly zero
    S0 = S.copy()
    S0[2, 2] = 0.0
    H, _ = nn.nnls_cd(S0, B, np.ones_like(B))
    assert (H[:, 2] == 0).all() and np.isfinite(H).all()
    Y, d, dead = nn.normalise(np.array([[1.0, 0.0, 3.0], [3.0, 0.0, 1.0]]))
    assert np.array_equal(d, [4.0, 0.0, 4.0]) and dead == 1 and np.array_equal(Y[:, 1], [0.0, 0.0]) and np.isfinite(Y).all()
    r = np.random.default_rng(5)
    Z = r.random((1500, 3))
    assert np.abs(nn.colsum_chunked(Z) - Z.sum(axis=0)).max() <= 1500 * nc.U * Z.sum(axis=0).max()


def test_restatement_factorises_the_planted_matrix():
    A, W0 = nc.planted()
    r = nn.nmf(A, 4, W0, track_loss=True)
    rel = r["loss"] / (A.data ** 2).sum()
    print("planted: iterations", r["iterations"], "delta", r["delta"], "relative loss", rel)
    assert r["converged"] and r["iterations"] < 30 and rel[-1] < 1e-3 and (np.diff(r["loss"]) <= 0).all() and r["dead"] == 0
    assert np.abs(r["w"].sum(axis=0) - 1).max() < 1e-12 and np.abs(r["h"].sum(axis=1) - 1).max() < 1e-12


# ------------------------------------------------------------------ plumbing
def test_header_and_loader_name_the_same_entries():
    from gficf_amd import _nmf_lib as lib

    text = open(os.path.join(ROOT, "include", "gficf_nmf.h")).read()
    body = text[text.index("extern \"C\""):]
    declared = re.findall(r"\b(gficf_n(?:mf|nls)_\w+)\s*\(([^;]*)\)\s*;", body)
    assert set(n for n, _ in declared) == set(lib.SIGNATURES) and len(declared) == 10
    for name, args in declared:
        n = 0 if args.strip() == "void" else args.count(",") + 1
        assert n == len(lib.SIGNATURES[name][1]), name
    assert "#define GFICF_NMF_ABI_VERSION 1" in text and lib.ABI_VERSION == 1
    assert re.search(r"#define\s+GFICF_NMF_MAX_K\s+128\b", text) and lib.MAX_K == 128 == gficf_amd.api.NMF_MAX_K
    assert re.search(rf"#define\s+GFICF_NMF_NNLS_WS_BYTES\s+{lib.NNLS_WS_BYTES}\b", text)
    assert [lib.ld(k) for k in (1, 8, 9, 128)] == [8, 8, 16, 128] and [lib.lp(k) for k in (1, 16, 17, 33, 65, 128)] == [16, 16, 32, 64, 128, 128]
    core = open(os.path.join(ROOT, "include", "gficf_hip.h")).read()
    assert re.search(r"#define\s+GFICF_HIP_ABI_VERSION\s+7\b", core)


def test_makefile_builds_the_library_with_the_others():
    csrc = os.path.join(ROOT, "gficf_amd", "csrc")
    text = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^ADDONS\s*:=.*\bnmf\b", text, re.M) and "libgficf_nmf.so" in text[:text.index("HIPCC")]
    assert re.search(r"^nmf\.o: \.\./\.\./include/gficf_nmf\.h pca_kernels\.h addon_status\.h block_ops\.h$", text, re.M)
    assert re.search(r"^nmf\.o: HIPFLAGS \+= -ffp-contract=off$", text, re.M)
    build = subprocess.run(["make", "-n", "-B", "-C", csrc, "all"], capture_output=True, text=True, check=True).stdout.splitlines()
    link = [ln for ln in build if " -o ../libgficf_nmf.so " in ln]
    assert len(link) == 1 and re.search(r"hipcc --offload-arch=gfx950 -shared -fPIC -o \.\./libgficf_nmf\.so nmf\.o -L\.\. -lgficf_hip\b", link[0])
    comp = [ln for ln in build if ln.endswith(" -o nmf.o")]
    assert len(comp) == 1 and "-ffp-contract=off" in comp[0] and "--offload-arch=gfx950" in comp[0] and "fast-math" not in comp[0]
    clean = subprocess.run(["make", "-n", "-C", csrc, "clean"], capture_output=True, text=True, check=True).stdout
    assert re.search(r"^rm -f .*\bnmf\.o\b.* \.\./libgficf_nmf\.so\b", clean, re.M)


def test_loader(monkeypatch):
    from gficf_amd import _nmf_lib as lib

    L = lib.load()
    assert isinstance(L, ctypes.CDLL) and lib.load() is L and L.gficf_nmf_abi_version() == lib.ABI_VERSION
    for sym, (res, args) in lib.SIGNATURES.items():
        fn = getattr(L, sym)
        assert fn.restype is res and list(fn.argtypes) == list(args), sym
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert sorted(set(re.findall(r" T (gficf_[a-z0-9_]+)$", out, re.M))) == sorted(lib.SIGNATURES)
    wb = L.gficf_nmf_workspace_bytes
    assert wb(300, 200, 6000, 5) >= 8 * 300 * 8 and wb(300, 200, 6000, 5) == wb(200, 300, 6000, 5) and wb(300, 200, 6000, 100) > wb(300, 200, 6000, 5)
    assert wb(23000, 54000, 50_000_000, 100) < 2 << 30
    for bad in ((0, 200, 10, 5), (300, 0, 10, 5), (300, 200, -1, 5), (300, 200, 10, 0), (300, 200, 10, 129), (2 ** 31, 200, 10, 5), (300, 2 ** 31, 10, 5)):
        assert wb(*bad) == 0, bad
    assert wb(300, 1, 10, 128) > 0                              # one new cell against 128 factors: the projection takes it
    monkeypatch.setattr(lib, "LIB_PATH", os.path.join(os.path.dirname(lib.LIB_PATH), "libgficf_nmf_missing.so"))
    with pytest.raises(ImportError, match="not found: build it with"):
        lib.load()


def test_surface():
    p = inspect.signature(gficf_amd.nmf).parameters
    want = dict(seed=180582, W0=None, tol=1e-4, maxit=100, L1=(0.0, 0.0), cd_tol=1e-8, cd_maxit=100, ridge=1e-15, track_loss=False)
    assert list(p)[:2] == ["A", "k"] and {k: p[k].default for k in want} == want
    q = inspect.signature(gficf_amd.nnls).parameters
    assert list(q)[:3] == ["S", "B", "H0"] and (q["H0"].default, q["cd_tol"].default, q["cd_maxit"].default, q["ret_sweeps"].default) == (None, 1e-8, 100, False)
    r = inspect.signature(gficf_amd.runNMF).parameters
    assert list(r)[:2] == ["data", "dim"] and (r["dim"].default, r["seed"].default, r["use_odgenes"].default, r["n_odgenes"].default,
                                               r["var_scale"].default) == (None, 180582, False, None, False)
    assert list(inspect.signature(gficf_amd.nmf_loss).parameters)[:4] == ["A", "w", "d", "h"]
    assert list(inspect.signature(gficf_amd.nmf_project).parameters)[:2] == ["data_or_w", "gficf_new"]
    for name in ("nnls", "nmf_half", "nmf_loss", "nmf", "nmf_project", "nmf_workspace_bytes", "nmf_sync"):
        assert callable(getattr(gficf_amd.HipOps, name)), name


def test_stage_ops_refuse_a_tensor_of_another_pitch():
    """The stages index dense operands by the pitch ld(k): a tensor of another shape is refused before anything is enqueued."""
    import torch

    ops = gficf_amd.HipOps
    ops._nmf_dense(20, B=(torch.zeros(4, 24, dtype=torch.float64), 4), H0=(None, 4))
    for bad in (torch.zeros(4, 32, dtype=torch.float64), torch.zeros(3, 24, dtype=torch.float64), torch.zeros(4, 24, dtype=torch.float32), torch.zeros(96, dtype=torch.float64)):
        with pytest.raises(ValueError, match=r"B must be a \(4, 24\) float64 tensor for k = 20"):
            ops._nmf_dense(20, B=(bad, 4))
    with pytest.raises(ValueError, match="S must be a float64 matrix of at least 20 x 20"):
        ops.nnls(None, 20, torch.zeros(16, 32, dtype=torch.float64), torch.zeros(4, 24, dtype=torch.float64), None, 1e-8, 10, None, None, None)
    with pytest.raises(ValueError, match="sweeps must hold 4 int32"):
        ops._nmf_small(20, sweeps=torch.zeros(3, dtype=torch.int32), rows=4)
    with pytest.raises(ValueError, match=r"S must be \(32, 32\)"):
        ops._nmf_small(20, S=torch.zeros(24, 24, dtype=torch.float64))


def test_argument_checks():
    """Everything the mirror refuses, it refuses before it touches a device."""
    A = nc.sparse_300x200()
    for k in (0, 129, 201):
        with pytest.raises(ValueError, match="1 <= k <= min"):
            gficf_amd.nmf(A, k)
    neg = A.copy()
    neg.data[7] = -0.5
    with pytest.raises(ValueError, match="negative"):
        gficf_amd.nmf(neg, 3)
    with pytest.raises(ValueError, match="W0 must be G x k = 300 x 3"):
        gficf_amd.nmf(A, 3, W0=np.ones((300, 4)))
    with pytest.raises(ValueError, match="W0 holds a negative"):
        gficf_amd.nmf(A, 3, W0=-np.ones((300, 3)))
    for kw in (dict(tol=-1.0), dict(maxit=-1), dict(L1=(0.0, -1.0)), dict(cd_tol=-1.0), dict(cd_maxit=-1), dict(ridge=-1.0)):
        with pytest.raises(ValueError, match="may not be negative"):
            gficf_amd.nmf(A, 3, **kw)
    with pytest.raises(ValueError, match="S must be k x k"):
        gficf_amd.nnls(np.ones((2, 3)), np.ones((4, 2)))
    with pytest.raises(ValueError, match="B must be a matrix x 2"):
        gficf_amd.nnls(np.eye(2), np.ones((4, 3)))
    with pytest.raises(ValueError, match="H0 must be 4 x 2"):
        gficf_amd.nnls(np.eye(2), np.ones((4, 2)), H0=np.ones((3, 2)))
    with pytest.raises(ValueError, match="H0 holds a negative"):
        gficf_amd.nnls(np.eye(2), np.ones((4, 2)), H0=-np.ones((4, 2)))
    with pytest.raises(ValueError, match="First run runNMF"):
        gficf_amd.nmf_project({"pca": {"cells": np.zeros((3, 2))}}, A)
    with pytest.raises(ValueError, match="one row per row of w"):
        gficf_amd.nmf_project(np.ones((299, 3)), A)
    data = {"gficf": A, "rawCounts": A}
    with pytest.raises(NotImplementedError, match='use_odgenes="cr"'):
        gficf_amd.runNMF(data, dim=3, use_odgenes=True)
    with pytest.raises(NotImplementedError, match='var_scale="cr"'):
        gficf_amd.runNMF(data, dim=3, var_scale=True)
    with pytest.raises(ValueError, match="Raw Counts absent"):
        gficf_amd.runNMF({"gficf": A}, dim=3, use_odgenes="cr")
    with pytest.raises(ValueError, match="Specify the number of dims"):
        gficf_amd.runNMF({"gficf": A})


def test_pca_project_dispatches_on_type(monkeypatch):
    """data["pca"]["type"] == "NMF" routes pca_project to nmf_project; any other data never reaches it."""
    seen = []
    monkeypatch.setattr(gficf_amd.api, "nmf_project", lambda data, new, ctx=None: seen.append((data, new, ctx)) or "projected")
    new = sp.csc_matrix(np.ones((3, 2)))
    data = {"pca": {"type": "NMF", "genes": np.ones((3, 2)), "cells": np.ones((4, 2))}}
    assert gficf_amd.pca_project(data, new) == "projected" and seen[0][0] is data and seen[0][1] is new
    with pytest.raises(ValueError, match="First run runPCA"):
        gficf_amd.pca_project({}, new)
    # a data of runPCA / runLSA carries no "type": it goes on to the linear projection, which here needs the library's context
    calls = []
    monkeypatch.setattr(gficf_amd.api, "default_context", lambda: calls.append(1) or (_ for _ in ()).throw(RuntimeError("linear path")))
    with pytest.raises(RuntimeError, match="linear path"):
        gficf_amd.pca_project({"pca": {"genes": np.ones((3, 2)), "cells": np.ones((4, 2))}}, new)
    assert len(seen) == 1 and calls == [1]
