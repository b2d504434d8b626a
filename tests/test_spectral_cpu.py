"""No GPU: the numpy helpers of the spectral tests against what defines them, the header of libgficf_spectral.so against its
loader, and the argument handling of the Python mirror (everything it decides before the first call into the library)."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import gficf_amd
from gficf_amd import _spectral_lib
from gficf_amd.api import _spectral_args, _spectral_coordinates
from tests.helpers import spectral_block_np as sb
from tests.helpers import spectral_cases as sc
from tests.helpers import spectral_np as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ ABI
def test_header_and_loader_name_the_same_entries():
    text = open(os.path.join(ROOT, "include", "gficf_spectral.h")).read()
    body = text[text.index("extern \"C\""):]
    declared = re.findall(r"\b(gficf_(?:spectral|graph_components)_\w+)\s*\(([^;]*)\)\s*;", body)
    assert set(n for n, _ in declared) == set(_spectral_lib.SIGNATURES)
    for name, args in declared:
        n = 0 if args.strip() == "void" else args.count(",") + 1
        assert n == len(_spectral_lib.SIGNATURES[name][1]), name
    assert "#define GFICF_SPECTRAL_ABI_VERSION 1" in text and _spectral_lib.ABI_VERSION == 1
    assert re.search(r"#define\s+GFICF_SPECTRAL_MAX_NDIM\s+%d\b" % _spectral_lib.MAX_NDIM, text)
    assert re.search(r"#define\s+GFICF_SPECTRAL_MAX_M\s+%d\b" % _spectral_lib.MAX_M, text)
    core = open(os.path.join(ROOT, "include", "gficf_hip.h")).read()
    assert re.search(r"#define\s+GFICF_HIP_ABI_VERSION\s+7\b", core)
    umap = open(os.path.join(ROOT, "include", "gficf_umap.h")).read()
    assert "#define GFICF_UMAP_ABI_VERSION 1" in umap


def test_makefile_builds_the_library_with_the_others():
    # what make itself would run (a dry run of everything, nothing is compiled): the rules are free to be shared with the other add-ons
    csrc = os.path.join(ROOT, "gficf_amd", "csrc")
    build = subprocess.run(["make", "-n", "-B", "-C", csrc, "all"], capture_output=True, text=True, check=True).stdout
    assert re.search(r"^\S*hipcc .* -o \.\./libgficf_spectral\.so spectral\.o -L\.\. -lgficf_hip\b", build, re.M)
    clean = subprocess.run(["make", "-n", "-C", csrc, "clean"], capture_output=True, text=True, check=True).stdout
    assert re.search(r"^rm -f .*\bspectral\.o\b.* \.\./libgficf_spectral\.so\b", clean, re.M)


# ------------------------------------------------------------------------------------------------ helper self-checks
@pytest.mark.parametrize("N,s", [(300, 3), (64, 2), (33, 1)])
def test_ring_has_its_closed_form_spectrum(N, s):
    P = sn.ring(N, s)
    assert P.dtype == np.float32 and (np.diff(P.indptr) == 2 * s).all() and (P != P.T).nnz == 0
    w, U, q0 = sn.spectrum(P)
    assert abs(w[0] - 1.0) < 1e-12 and abs(abs(U[:, 0] @ q0) - 1.0) < 1e-12
    assert abs(w[1] - sn.ring_value(N, s)) < 1e-12 and abs(w[2] - sn.ring_value(N, s)) < 1e-12      # the doubly degenerate top plane
    assert w[3] < w[2] - 1e-6 and abs(w[3] - sn.ring_value(N, s, 2)) < 1e-12
    r = np.sqrt((U[:, 1:3] ** 2).sum(axis=1))
    assert np.allclose(r, np.sqrt(2.0 / N), rtol=1e-9)                                                # every point at radius sqrt(2 / N)
    assert sn.ring_value(300, 3) == pytest.approx(0.99897674733, abs=1e-11)


def test_dense_operator_and_residuals():
    P = sn.ring(20, 2).tolil()
    P[0, 7] = P[7, 0] = 3.0
    P = P.tocsr()
    S, q0 = sn.dense_operator(P)
    assert np.allclose(S, S.T) and np.allclose(S @ q0, q0, atol=1e-14)
    w, U, _ = sn.spectrum(P)
    assert (np.diff(w) <= 0).all() and sn.residuals(P, U[:, 1:3], w[1:3]).max() < 1e-13
    assert sn.davis_kahan(w, 1, 1e-6) == pytest.approx(1e-6 / min(w[0] - w[1], w[1] - w[2]))
    assert sn.sine(U[:, 1], U[:, 1]) < 1e-15 and sn.sine(U[:, 1], U[:, 2]) == pytest.approx(1.0)
    assert sn.subspace_gap(U[:, 1:3], U[:, 1:3] @ np.array([[0.6, -0.8], [0.8, 0.6]])) < 1e-7


def test_canonical_sign():
    V = np.array([[0.1, -0.5], [-0.7, 0.5], [0.7, 0.2]])
    got = sn.canonical_sign(V)
    assert np.array_equal(got[:, 0], -V[:, 0]) and np.array_equal(got[:, 1], -V[:, 1])               # ties: the lowest index decides
    assert np.array_equal(sn.canonical_sign(got), got)


def test_components_relabel_to_the_smallest_id():
    P = sp.lil_matrix((7, 7), dtype=np.float32)
    P[5, 2] = 1                                                                                       # stored one way only
    P[2, 6] = 1
    P[1, 4] = P[4, 1] = 1
    lab, n = sn.components(P.tocsr())
    assert n == 4 and lab.dtype == np.int32 and lab.tolist() == [0, 1, 2, 3, 1, 2, 2]


def test_eigh_start_draws_the_noise_second():
    P = sn.ring(40, 2)
    Y = sn.eigh_start(P, 5)
    rng = np.random.default_rng(5)
    rng.standard_normal((40, 2))
    noise = rng.normal(0.0, 1e-4, size=(40, 2))
    assert abs(np.abs(Y - noise).max() - 10.0) < 1e-12
    raw = sn.eigh_start(P, 5, jitter=False)
    assert np.allclose(np.linalg.norm(raw, axis=0), 1.0) and np.allclose((Y - noise) * np.abs(raw).max() / 10.0, raw)
    assert np.array_equal(_spectral_coordinates(raw, np.random.default_rng(0), False), raw)


# ------------------------------------------------------------------------------------------------ the mirror's argument handling
def test_argument_checks_of_the_mirror():
    P = sn.ring(12, 1)
    for kw in ({"ndim": 0}, {"ndim": 9}, {"ndim": 12}, {"m": 5}, {"m": 65}, {"tol": 0.0}, {"tol": np.inf}, {"max_restarts": -1},
               {"start": np.zeros((12, 3))}, {"start": np.full((12, 2), np.nan)}):
        with pytest.raises(ValueError):
            gficf_amd.spectral_embedding(P, **kw)
    with pytest.raises(ValueError, match="square"):
        gficf_amd.spectral_embedding(sp.csr_matrix((3, 4), dtype=np.float32))
    with pytest.raises(ValueError, match="square"):
        gficf_amd.graph_components(sp.csr_matrix((3, 4), dtype=np.float32))
    with pytest.raises(ValueError, match="exceed"):
        gficf_amd.spectral_init(sn.ring(2, 1))
    assert _spectral_args(12, 2, 32, 1e-4, 200, None) == (2, 32, 200, None)
    assert _spectral_args(12, 8, 18, 1e-4, 0, None)[:3] == (8, 18, 0)
    X = np.random.default_rng(0).standard_normal((30, 4))
    with pytest.raises(ValueError, match="init"):
        gficf_amd.umap(X, "laplacian")
    with pytest.raises(ValueError, match="metric"):
        gficf_amd.umap(X, "spectral", metric="hamming")


def test_run_reduction_still_refuses_spectral_and_names_the_way():
    data = {"pca": {"cells": np.random.default_rng(1).standard_normal((40, 5))}}
    with pytest.raises(NotImplementedError, match="spectral") as e:
        gficf_amd.runReduction(data, init="spectral", verbose=False)
    assert "gficf_amd.umap(" in str(e.value) and "spectral_init" in str(e.value)
    assert gficf_amd.api._REDUCTION_KW["init"] == "pca"


# ------------------------------------------------------------------------------------------------ the new graphs and bounds
def test_planted_graph_is_all_hubs_with_a_gap_after_eight():
    P, w, U, q0, _ = sc.graph("planted")
    assert P.shape == (1100, 1100) and P.dtype == np.float32 and (P != P.T).nnz == 0 and P.has_sorted_indices
    assert (np.diff(P.indptr) == 1099).all() and P.diagonal().max() == 0
    assert (np.diff(P.indptr) > sn.HUB_LEN).sum() > sn.HUB_WAVES                                      # the strided hub loop runs
    assert abs(w[0] - 1.0) < 1e-12 and 0.5804 - 1e-4 <= w[8] <= w[1] <= 0.5844 + 1e-4
    assert w[8] - w[9] > 0.56 and abs(w[9] - 0.019) < 1e-3


def test_threshold_graph_has_rows_on_both_sides_of_the_hub_length():
    P, w, U, q0, _ = sc.graph("threshold")
    n = np.diff(P.indptr)
    assert P.dtype == np.float32 and (P != P.T).nnz == 0 and P.has_sorted_indices and (P.data == 1).all()
    assert (n == sn.HUB_LEN).sum() == 598 and np.flatnonzero(n == sn.HUB_LEN + 1).tolist() == [0, 300]
    assert abs(w[0] - 1.0) < 1e-12
    assert np.allclose(w[1:5], [0.72331, 0.72326, 0.15847, 0.15845], atol=1e-5)
    gaps = -np.diff(w[1:7])
    assert 2e-5 <= gaps[0::2].min() and gaps[0::2].max() < 1e-4 and gaps[1::2].min() > 1e-2           # near-degenerate pairs, the smallest gap 2e-5


def test_outside_cluster_and_subspace_sine_meet_their_bounds():
    P, w, U, q0, S = sc.graph("ring-300-3")
    rng = np.random.default_rng(0)
    # a unit vector in the top plane plus a little of everything else: what lies outside the plane obeys residual / delta
    x = U[:, 1:3] @ np.array([0.6, 0.8]) + 1e-5 * (U @ rng.standard_normal(300))
    x /= np.linalg.norm(x)
    theta = float(x @ S @ x)
    r = float(np.linalg.norm(S @ x - theta * x))
    outside = np.abs(w - w[1]) > 1e-9
    assert (~outside).sum() == 2
    delta = float(np.abs(w[outside] - theta).min())
    got = sn.outside_cluster(x, theta, w, U, delta)
    assert 1e-6 < got <= r / delta and got == pytest.approx(np.linalg.norm(np.delete(U, [1, 2], axis=1).T @ x), rel=1e-6)
    assert sn.outside_cluster(U[:, 1], w[1], w, U, delta) < 1e-14                                     # not 1e-8: from the remainder
    # a slightly tilted copy of the leading four vectors, each degenerate plane turned within itself
    turn = np.kron(np.eye(2), np.array([[0.6, -0.8], [0.8, 0.6]]))
    Q, _ = np.linalg.qr(U[:, 1:5] @ turn + 1e-6 * rng.standard_normal((300, 4)))
    th = np.diag(Q.T @ S @ Q).copy()
    res = np.linalg.norm(S @ Q - Q * th[None, :], axis=0)
    got, bound = sn.subspace_sine(Q, U[:, 1:5]), sn.subspace_bound(w, th, res)
    assert 1e-7 < got <= bound and bound < 1.0
    assert got == pytest.approx(np.linalg.norm(np.delete(U, [1, 2, 3, 4], axis=1).T @ Q, 2), rel=1e-6)
    assert sn.subspace_sine(U[:, 1:5], U[:, 1:5]) < 1e-14
    sep = min(w[0] - th.max(), th.min() - w[5])
    assert bound == pytest.approx(np.linalg.norm(res) / sep)


# ------------------------------------------------------------------------------------------------ the method in numpy
@pytest.mark.parametrize("case", sc.MATRIX, ids=sc.case_id)
def test_block_method_converges_over_the_matrix(case):
    """Every case of tests/test_spectral_ndim_gpu.py is solvable by the header's method within 200 restarts, to the device's checks."""
    name, ndim, m, tol = case
    r = sc.port(name, ndim, m, tol)
    print(f"{sc.case_id(case)}: {r['restarts']} restarts, {r['multiplications']} multiplications")
    sc.check_against_eigh(name, r, tol)
    if name == "ring-300-3":
        want = [sn.ring_value(300, 3, 1 + l // 2) for l in range(ndim)]
        assert np.abs(r["values"] - want).max() <= 1e-12


@pytest.mark.parametrize("case", sc.SMALL, ids=sc.case_id)
def test_block_method_on_small_graphs_needs_no_restart(case):
    """mc = N - 1: the basis spans the whole complement of q0, the narrower last block stays."""
    name, ndim, m, tol = case
    r = sc.port(name, ndim, m, tol)
    sc.check_against_eigh(name, r, tol)
    assert r["restarts"] == 0 and np.abs(r["values"] - sc.graph(name)[1][1:1 + ndim]).max() <= 1e-12


STALLS = [(3, 32), (2, 33)]


@pytest.mark.parametrize("ndim,m", STALLS)
def test_narrow_last_block_stalls(ndim, m):
    """The rule the header used to state: a cycle capped by m ends in a narrower block.  Not converged after 200 restarts."""
    r = sc.port("blobs", ndim, m, 1e-4, True)
    print(f"ndim {ndim}, m {m}: residuals {r['residuals']} after {r['restarts']} restarts")
    assert not r["converged"] and r["restarts"] == sc.MAX_RESTARTS
    assert (r["residuals"] > 1e-4 * np.abs(r["values"])).any()


@pytest.mark.parametrize("ndim,m", STALLS)
def test_full_last_block_converges_where_the_narrow_one_stalls(ndim, m):
    """Why the rule exists: the same two cases, a cycle ended at its last full block (4 and 2 restarts when this was written)."""
    r = sc.port("blobs", ndim, m, 1e-4)
    print(f"ndim {ndim}, m {m}: {r['restarts']} restarts")
    assert r["converged"] and r["restarts"] <= 10


def test_block_method_drops_a_duplicated_start_column_and_refuses_q0():
    P, w, U, q0, S = sc.graph("blobs")
    g, h = np.random.default_rng(7).standard_normal((2, 1200))
    for start, most in ((np.stack([g, g], axis=1), 10), (np.stack([g, g, h], axis=1), 12)):
        r = sc.as_result(sb.solve(P, start.shape[1], start, 1e-4, 32, sc.MAX_RESTARTS))
        print(f"duplicated column, ndim {start.shape[1]}: {r['restarts']} restarts")
        sc.check_against_eigh("blobs", r, 1e-4)
        assert r["restarts"] <= most
    with pytest.raises(ValueError, match="spans 0 directions"):
        sb.solve(P, 2, np.stack([q0, -3.0 * q0], axis=1), 1e-4, 32, sc.MAX_RESTARTS)
