"""CPU: the numpy port of the randomized SVD (tests/helpers/rsvd_np.py) against LAPACK, closed forms and itself; the elbow
rule of computePCADim; the exported surface of libgficf_pca.so; argument errors of the Python mirror."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.helpers import rsvd_np as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _omega(n, l, seed=7):
    return np.random.default_rng(seed).standard_normal((n, l))


def _dense_svd(M, k, centre=False):
    A = M.T.toarray()
    if centre:
        A = A - A.mean(axis=0)
    U, d, Vt = np.linalg.svd(A, full_matrices=False)
    V = Vt.T[:, :k]
    s = rp.sign_rule(V)
    return {"d": d[:k], "cells": U[:, :k] * d[:k] * s, "genes": V * s, "d_all": d}


# both orientations: N > G and N < G
PLANTED = {"cells_tall": (600, 240, 6), "genes_tall": (240, 600, 6)}


@pytest.mark.parametrize("shape", sorted(PLANTED))
@pytest.mark.parametrize("centre", [False, True])
@pytest.mark.parametrize("variant", ["lapack", "gram"])
def test_port_matches_the_dense_svd_on_planted_matrices(shape, centre, variant):
    N, G, C = PLANTED[shape]
    M = rp.planted_sparse(N, G, C, seed=11)
    k, l = C, C + 10
    r = rp.rsvd(M, _omega(min(N, G), l), k, q=2, centre=centre, variant=variant)
    rp.assert_separated(r["d_all"], k)
    want = _dense_svd(M, k, centre)
    # the sketch against the exact decomposition: with g = d[k] / d[k - 1] of the exact values (about 0.25 as planted, 0.57
    # once centring has folded the programmes' common mean away), q = 2 power iterations leave the k leading vectors with
    # an error of g^(2q + 1) at worst and the values, which are stationary in the vectors, with its square
    g = want["d_all"][k] / want["d_all"][k - 1]
    dev = rp.deviations(want, r)
    assert dev["d"] < g ** 10 and dev["cells"] < g ** 5 and dev["genes"] < g ** 5, (g, dev)
    assert r["cells"].shape == (N, k) and r["genes"].shape == (G, k)
    assert (np.diff(r["d"]) <= 0).all()
    i = np.argmax(np.abs(r["genes"]), axis=0)
    assert (r["genes"][i, np.arange(k)] > 0).all()
    if centre:
        assert np.allclose(r["centre"], M.toarray().mean(axis=1), rtol=1e-13, atol=0)


@pytest.mark.parametrize("shape", sorted(PLANTED))
def test_the_two_variants_agree(shape):
    N, G, C = PLANTED[shape]
    M = rp.planted_sparse(N, G, C, seed=12)
    for centre in (False, True):
        _, _, dev = rp.variant_deviation(M, _omega(min(N, G), C + 10), C, 2, centre)
        assert max(dev.values()) < 1e-11, dev


@pytest.mark.parametrize("variant", ["lapack", "gram"])
@pytest.mark.parametrize("transposed", [False, True])
def test_port_matches_the_blocks_closed_form_at_rank_below_l(variant, transposed):
    # 4 blocks: d = a sqrt(n g) = 3 sqrt(60 * 20), 2 sqrt(50 * 30), 1.5 sqrt(40 * 25), 1 sqrt(30 * 10): 103.9, 77.5, 47.4, 17.3
    N, G = (200, 100) if not transposed else (200, 260)
    M, d, U, V = rp.blocks(N, G, [60, 50, 40, 30], [20, 30, 25, 10], [3.0, 2.0, 1.5, 1.0])
    l = 12                                                # rank 4 < l
    r = rp.rsvd(M, _omega(min(N, G), l), 4, q=2, variant=variant)
    assert np.isfinite(r["d_all"]).all() and np.isfinite(r["cells"]).all() and np.isfinite(r["genes"]).all()
    assert np.allclose(r["d"], d, rtol=1e-12, atol=0)
    assert np.abs(r["d_all"][4:]).max() <= 1e-12 * d[0]   # the trailing values of an exact-rank matrix are negligible
    assert np.allclose(r["genes"], V, rtol=0, atol=1e-12)  # V >= 0: already signed as the rule wants
    assert np.allclose(r["cells"], U * d, rtol=0, atol=1e-12 * d[0])


def test_orth_variants_span_the_same_range_and_drop_null_directions():
    rng = np.random.default_rng(3)
    Y = rng.standard_normal((300, 5)) @ rng.standard_normal((5, 9))      # rank 5, l = 9
    Q = rp.orth_gram(Y)
    assert np.isfinite(Q).all()
    assert np.abs(Q.T @ Q - np.diag([1.0] * 5 + [0.0] * 4)).max() < 1e-13
    Ql = rp.orth_lapack(Y[:, :5])
    assert rp.projector_diff(Q, Ql) < 1e-13


# ------------------------------------------------------------------------------------------------ computePCADim's rule
def _d_from_shares(ev):
    return np.sqrt(np.asarray(ev, dtype=np.float64))


def test_elbow_rule_on_hand_worked_vectors():
    from gficf_amd import pca_dim_rule

    # shares (they sum to 1):      .40  .25  .15  .09  .05  .03  .02  .01
    # diff:                           -.15 -.10 -.06 -.04 -.02 -.01 -.01
    # ratio to the first diff:         1   .667 .4   .267 .133 .067 .067
    # which(ratio < .1), 1-based: w = 6, 7;  diff(w) == 1: T;  cumsum = 1: never > 1 -> NA
    assert pca_dim_rule(_d_from_shares([.40, .25, .15, .09, .05, .03, .02, .01])) is None
    # shares:  .50  .20  .10  .06  .04  .03  .025 .02  .015 .01
    # diff:       -.30 -.10 -.04 -.02 -.01 -.005 -.005 -.005 -.005
    # ratio:       1   .333 .133 .0667 .0333 .0167 .0167 .0167 .0167
    # w = 4, 5, 6, 7, 8, 9;  diff(w) == 1: T T T T T;  cumsum = 1 2 3 4 5;  first > 1 at ix = 2 -> w[2] = 5
    assert pca_dim_rule(_d_from_shares([.50, .20, .10, .06, .04, .03, .025, .02, .015, .01])) == 5
    # the run-of-consecutive-indices quirk: isolated hits count nothing, and the cumsum does not reset between runs
    # shares:  .400 .200 .190 .100 .095 .010 .003 .002
    # diff:        -.2  -.01 -.09 -.005 -.085 -.007 -.001
    # ratio:        1   .05  .45  .025  .425  .035  .005
    # w = 2, 4, 6, 7;  diff(w) == 1: F F T;  cumsum = 0 0 1 -> NA
    assert pca_dim_rule(_d_from_shares([.400, .200, .190, .100, .095, .010, .003, .002])) is None
    # the same with one more small step: shares .400 .200 .190 .100 .095 .010 .003 .0015 .0005
    # ratio: 1 .05 .45 .025 .425 .035 .0075 .005;  w = 2, 4, 6, 7, 8;  diff == 1: F F T T;  cumsum = 0 0 1 2;  ix = 4 -> w[4] = 7
    assert pca_dim_rule(_d_from_shares([.400, .200, .190, .100, .095, .010, .003, .0015, .0005])) == 7
    # the rule sees shares, not magnitudes
    assert pca_dim_rule(1e3 * _d_from_shares([.50, .20, .10, .06, .04, .03, .025, .02, .015, .01])) == 5
    assert pca_dim_rule([3.0]) is None


# ------------------------------------------------------------------------------------------------ the library's surface
def _header_functions(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gficf_[a-z0-9_]+)\s*\(", src)))


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(re.findall(r" T (gficf_[a-z0-9_]+)$", out, re.M)))


def test_pca_library_exports_exactly_its_header():
    from gficf_amd import _pca_lib

    names = _header_functions("gficf_pca.h")
    assert len(names) == 11
    assert sorted(_pca_lib.SIGNATURES) == names
    L = _pca_lib.load()
    assert L.gficf_pca_abi_version() == 1
    if shutil.which("nm"):
        assert _exports(_pca_lib.LIB_PATH) == names
    # about 12 B per stored entry (the gene-major view) plus the dense operands
    assert L.gficf_rsvd_workspace_bytes(2000, 5000, 1_000_000, 60) > 12 * 1_000_000 + 4 * 5000 * 64 * 8 // 2
    assert L.gficf_rsvd_workspace_bytes(-1, 5000, 1000, 60) == 0 and L.gficf_rsvd_workspace_bytes(10, 10, 10, 129) == 0
    assert L.gficf_csc_tmm_workspace_bytes(100, 100, 1000, 0) == 0 and L.gficf_orthonormalize_workspace_bytes(100, 200) == 0
    assert L.gficf_csc_tmm_workspace_bytes(100, 100, 1000, 17) > 0 and L.gficf_orthonormalize_workspace_bytes(100, 17) > 0


def test_core_library_is_unchanged_85_symbols_abi_7():
    from gficf_amd import _lib

    L = _lib.load()
    assert L.gficf_hip_abi_version() == 7
    if shutil.which("nm"):
        assert len(_exports(_lib.LIB_PATH)) == 85


# ------------------------------------------------------------------------------------------------ the Python mirror
def test_argument_errors_of_runpca_runlsa_computepcadim():
    import scipy.sparse as sp

    import gficf_amd

    data = {"gficf": sp.csc_matrix(np.eye(4))}
    for fn in (gficf_amd.runPCA, gficf_amd.runLSA):
        with pytest.raises(ValueError, match="Specify the number of dims or run computePCADim first"):
            fn(dict(data))
        with pytest.raises(ValueError, match="Raw Counts absent"):
            fn(dict(data), dim=2, use_odgenes=True)
        with pytest.raises(NotImplementedError, match="findOverDispersed"):
            fn(dict(data, rawCounts=data["gficf"]), dim=2, use_odgenes=True)
        with pytest.raises(NotImplementedError, match="findOverDispersed"):
            fn(dict(data), dim=2, var_scale=True)
        with pytest.raises(NotImplementedError, match="randomized=True"):
            fn(dict(data), dim=2, randomized=False)
        d = dict(data)
        with pytest.raises(NotImplementedError):
            fn(d, dim=3, randomized=False)
        assert d["dimPCA"] == 3                             # stored before the decomposition, as in the reference
    with pytest.raises(NotImplementedError, match="randomized=True"):
        gficf_amd.computePCADim(dict(data), randomized=False)
    with pytest.raises(ValueError, match="First run runPCA or runLSA"):
        gficf_amd.pca_project({}, data["gficf"])
    with pytest.raises(ValueError, match="one row per row"):
        gficf_amd.pca_project({"pca": {"genes": np.zeros((5, 2)), "centre": False}}, data["gficf"])
    with pytest.raises(ValueError, match="omega must have"):
        gficf_amd.rsvd(data["gficf"], 2, omega=np.zeros((3, 2)))
    with pytest.raises(ValueError, match="one row per row of A"):
        gficf_amd.csc_tmm(data["gficf"], np.zeros((3, 2)))


def _no_device():
    import gficf_amd

    return gficf_amd.device_count() == 0


@pytest.mark.skipif(not _no_device(), reason="GPU present")
def test_entries_fail_with_no_device_without_a_gpu():
    import scipy.sparse as sp

    import gficf_amd

    M = sp.csc_matrix(np.eye(6))
    for call in (lambda: gficf_amd.rsvd(M, 2, p=2), lambda: gficf_amd.csc_tmm(M, np.ones((6, 2))),
                 lambda: gficf_amd.runPCA({"gficf": M}, dim=2),
                 lambda: gficf_amd.pca_project({"pca": {"genes": np.ones((6, 2)), "centre": False}}, M)):
        with pytest.raises(gficf_amd.GficfError) as e:
            call()
        assert e.value.status == "GFICF_ERR_NO_DEVICE"
