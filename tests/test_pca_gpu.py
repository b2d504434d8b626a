"""GPU: libgficf_pca.so (Y = A'X, orth, the randomized SVD, the projection) and its Python mirror against scipy and the numpy
port of tests/helpers/rsvd_np.py, given the same test matrix Omega.

Tolerance rule against the port.  The yardstick is the port's LAPACK variant.  On every input the port's two variants (LAPACK
QR / SVD and the Gram / eigh form) were run on the CPU and their largest deviation recorded, separately for d relative to d[0],
sign-aligned cells / d[0], sign-aligned genes, and (orth) the projector difference: MEASURED below.  That deviation is the size
of a legitimate difference between two correct f64 evaluations that orthonormalise differently; the test constant is 32 x it,
never below 64 eps (rsvd_np.tolerance).  No component is excluded: the inputs are planted so that every kept value is separated
from its neighbours by at least 10 %, which is asserted on the port's d."""
import numpy as np
import pytest
import scipy.sparse as sp

import gficf_amd
from gficf_amd import GficfError, synth
from gficf_amd.api import HipOps
from tests.helpers import rsvd_np as rp

pytestmark = pytest.mark.gpu

EPS = rp.EPS


def _omega(n, l, seed=7):
    return np.random.default_rng(seed).standard_normal((n, l))


# ------------------------------------------------------------------------------------------------ Y = A'X
def _gamma(n):
    return n * EPS / (1 - n * EPS)


def _sparse(nrows, ncols, density, seed, empty_every=7, zero_every=11):
    """CSC with empty columns and explicitly stored zeros."""
    rng = np.random.default_rng(seed)
    A = sp.random(nrows, ncols, density=density, format="csc", random_state=rng, data_rvs=rng.standard_normal)
    A = sp.csc_matrix(A.toarray() * (np.arange(ncols) % empty_every != 3))       # every 7th column empty
    A.sort_indices()
    A.data[::zero_every] = 0.0                                                   # stored zeros stay stored
    assert (np.diff(A.indptr) == 0).any() and (A.data == 0).any()
    return A


def _tmm_check(A, X, Y, exact=True):
    """|got - want| <= gamma_n sum |a||x| per element, n the column's entry count (the bound of any order of n fused or
    unfused multiply-adds; derived, not measured).  exact: want in extended precision, else scipy's f64 product."""
    n = np.diff(A.indptr)
    if exact:
        want = (A.T.toarray().astype(np.longdouble) @ X.astype(np.longdouble)).astype(np.float64)
    else:
        want = A.T @ X
    bound = _gamma(np.maximum(n, 1))[:, None] * (abs(A).T @ np.abs(X))
    err = np.abs(Y - want)
    assert (err <= bound).all(), float((err - bound).max())
    assert (Y[n == 0] == 0).all()


@pytest.mark.parametrize("l", [1, 17, 60, 64, 65, 128])
def test_csc_tmm_against_scipy(l):
    A = _sparse(700, 500, 0.03, seed=100 + l)
    X = np.random.default_rng(l).standard_normal((700, l))
    Y = gficf_amd.csc_tmm(A, X)
    assert Y.shape == (500, l)
    _tmm_check(A, X, Y)
    A64 = sp.csc_matrix((A.data, A.indices, A.indptr.astype(np.int64)), shape=A.shape)
    A32 = sp.csc_matrix((A.data, A.indices, A.indptr.astype(np.int32)), shape=A.shape)
    Y64, Y32 = gficf_amd.csc_tmm(A64, X), gficf_amd.csc_tmm(A32, X)
    assert np.array_equal(Y64, Y) and np.array_equal(Y32, Y)                     # both pointer widths, and the same bits again


def test_csc_tmm_long_column_is_cut_into_segments():
    nrows = 200_000
    rng = np.random.default_rng(5)
    few = np.sort(rng.choice(nrows, 5, replace=False))
    indptr = np.array([0, nrows, nrows + 5, nrows + 5, nrows + 5 + 1500], dtype=np.int64)
    mid = np.sort(rng.choice(nrows, 1500, replace=False))                        # 1500 entries: two segments, the second short
    indices = np.concatenate([np.arange(nrows), few, mid]).astype(np.int32)
    A = sp.csc_matrix((rng.standard_normal(len(indices)), indices, indptr), shape=(nrows, 4))
    X = rng.standard_normal((nrows, 17))
    Y = gficf_amd.csc_tmm(A, X)
    _tmm_check(A, X, Y)
    assert np.array_equal(gficf_amd.csc_tmm(A, X), Y)


def test_csc_tmm_more_than_ten_million_entries():
    nrows, ncols, per = 20_000, 6_000, 1_800
    rng = np.random.default_rng(6)
    indices = rng.integers(0, nrows, ncols * per, dtype=np.int32)
    A = sp.csc_matrix((rng.standard_normal(ncols * per), indices, np.arange(ncols + 1, dtype=np.int64) * per), shape=(nrows, ncols))
    A.sum_duplicates()                                                           # canonical before the first call: scipy would do it in place later
    assert A.nnz > 10_000_000
    X = rng.standard_normal((nrows, 8))
    Y = gficf_amd.csc_tmm(A, X)
    _tmm_check(A, X, Y, exact=False)
    assert np.array_equal(gficf_amd.csc_tmm(A, X), Y)


def test_hipops_csc_tmm_equals_the_host_form():
    import torch

    A = _sparse(700, 500, 0.03, seed=9)
    X = np.random.default_rng(9).standard_normal((700, 33))
    ops = HipOps(0)
    dev = torch.device("cuda", 0)
    cp, ri, xv = (torch.from_numpy(a).to(dev) for a in (A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data))
    Xd = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev)
    Yd = torch.zeros((33, 500), dtype=torch.float64, device=dev)
    ws = torch.empty(ops.csc_tmm_workspace_bytes(700, 500, A.nnz, 33), dtype=torch.uint8, device=dev)
    ops.csc_tmm(700, 500, cp, ri, xv, Xd, 33, ws, Yd)
    ops.rsvd_sync(ws)
    assert np.array_equal(Yd.cpu().numpy().T, gficf_amd.csc_tmm(A, X))


# ------------------------------------------------------------------------------------------------ orth
def _orth_input(name):
    rng = np.random.default_rng({"decay": 1, "rank_deficient": 2, "square": 3, "l128": 4}[name])
    if name == "decay":                                   # 40 columns, singular values from 1 down to 1e-3
        return rng.standard_normal((3000, 40)) * np.logspace(0, -3, 40), 40
    if name == "rank_deficient":                          # rank 10 < l = 24
        return rng.standard_normal((2000, 10)) @ rng.standard_normal((10, 24)), 10
    if name == "square":                                  # m = l
        return rng.standard_normal((32, 32)) + 6 * np.eye(32), 32
    return rng.standard_normal((4000, 128)), 128


# projector difference between the port's two variants on these inputs, measured on the CPU
ORTH_MEASURED = {"decay": 3.2e-17, "rank_deficient": 3.9e-17, "square": 1.5e-15, "l128": 7.7e-17}


def _gpu_orth(Y):
    import torch

    m, l = Y.shape
    ops = HipOps(0)
    dev = torch.device("cuda", 0)
    Yd = torch.from_numpy(np.ascontiguousarray(Y.T)).to(dev)
    ws = torch.empty(ops.orthonormalize_workspace_bytes(m, l), dtype=torch.uint8, device=dev)
    ops.orthonormalize(m, l, Yd, ws)
    ops.rsvd_sync(ws)
    return Yd.cpu().numpy().T


@pytest.mark.parametrize("name", sorted(ORTH_MEASURED))
def test_orthonormalize(name):
    Y, rank = _orth_input(name)
    m, l = Y.shape
    Q = _gpu_orth(Y)
    assert np.isfinite(Q).all()
    # Q'Q = I on the kept directions, exactly zero columns for the dropped ones, which come last.  Bound: an m-term dot
    # product of unit vectors carries at most gamma_m, once in the library's second Gram matrix and once in numpy's check
    want = np.diag([1.0] * rank + [0.0] * (l - rank))
    assert np.abs(Q.T @ Q - want).max() <= 4 * max(m, 64) * EPS
    assert (Q[:, rank:] == 0).all()
    Ql = rp.orth_lapack(Y) if rank == l else rp.orth_gram(Y)      # (a rank-deficient Y: LAPACK's Q completes the basis arbitrarily)
    assert rp.projector_diff(Q, Ql) <= rp.tolerance(ORTH_MEASURED[name])
    assert np.array_equal(_gpu_orth(Y), Q)


# ------------------------------------------------------------------------------------------------ rsvd against the port
# name: (N, G, groups, k, l, q, centre)
RSVD_CASES = {
    "cells_tall":         (600, 240, 6, 6, 16, 2, False),
    "genes_tall":         (240, 600, 6, 6, 16, 2, False),
    "cells_tall_q0":      (600, 240, 6, 6, 16, 0, False),
    "genes_tall_q0":      (240, 600, 6, 6, 16, 0, False),
    "cells_tall_centre":  (600, 240, 6, 5, 16, 2, True),
    "genes_tall_centre":  (240, 600, 6, 5, 16, 2, True),
    "k1":                 (600, 240, 6, 1, 11, 2, False),
    "l128":               (600, 240, 6, 6, 128, 2, False),
    "genes_tall_l128":    (240, 600, 6, 6, 128, 1, True),
}
# deviation between the port's two variants on these inputs (d / d[0], cells / d[0], genes), measured on the CPU
RSVD_MEASURED = {
    "cells_tall":         {"d": 4.0e-16, "cells": 4.0e-16, "genes": 5.0e-16},
    "genes_tall":         {"d": 1.5e-15, "cells": 5.7e-16, "genes": 1.2e-15},
    "cells_tall_q0":      {"d": 6.4e-16, "cells": 3.4e-16, "genes": 7.5e-16},
    "genes_tall_q0":      {"d": 4.1e-16, "cells": 4.1e-15, "genes": 5.4e-15},
    "cells_tall_centre":  {"d": 5.0e-16, "cells": 2.2e-16, "genes": 1.5e-15},
    "genes_tall_centre":  {"d": 6.7e-16, "cells": 6.4e-16, "genes": 5.6e-16},
    "k1":                 {"d": 3.2e-16, "cells": 1.8e-16, "genes": 3.9e-16},
    "l128":               {"d": 6.4e-16, "cells": 4.2e-16, "genes": 3.1e-15},
    "genes_tall_l128":    {"d": 1.9e-15, "cells": 3.4e-16, "genes": 7.7e-16},
}


def _rsvd_input(name):
    N, G, C, k, l, q, centre = RSVD_CASES[name]
    return rp.planted_sparse(N, G, C, seed=21), _omega(min(N, G), l, seed=22), k, q, centre


def _against_port(got, want, measured):
    rp.assert_separated(want["d_all"], len(want["d"]))
    dev = rp.deviations(want, {"d": got["d"], "cells": got["cells"], "genes": got["v"]})
    for key in ("d", "cells", "genes"):
        assert dev[key] <= rp.tolerance(measured[key]), (key, dev[key], rp.tolerance(measured[key]))
    # the sign rule itself: no alignment here
    i = np.argmax(np.abs(got["v"]), axis=0)
    assert (got["v"][i, np.arange(got["v"].shape[1])] > 0).all()
    assert np.array_equal(np.sign(got["v"][i, np.arange(len(i))]), np.sign(want["genes"][i, np.arange(len(i))]))


@pytest.mark.parametrize("name", sorted(RSVD_CASES))
def test_rsvd_against_the_port(name):
    M, om, k, q, centre = _rsvd_input(name)
    got = gficf_amd.rsvd(M, k, q=q, omega=om, centre=centre)
    want = rp.rsvd(M, om, k, q, centre, "lapack")
    assert got["d"].shape == (k,) and got["cells"].shape == (M.shape[1], k) and got["v"].shape == (M.shape[0], k)
    assert (np.diff(got["d"]) <= 0).all()
    _against_port(got, want, RSVD_MEASURED[name])
    if centre:
        assert np.allclose(got["centre"], want["centre"], rtol=0, atol=_gamma(M.shape[1]) * np.abs(want["centre"]).max())
    else:
        assert got["centre"] is None
    again = gficf_amd.rsvd(M, k, q=q, omega=om, centre=centre)
    for key in ("d", "cells", "v"):
        assert np.array_equal(again[key], got[key]), key


@pytest.mark.parametrize("name", ["cells_tall_centre", "genes_tall"])
def test_rsvd_device_form_gives_the_host_form_bits(name):
    import torch

    M, om, k, q, centre = _rsvd_input(name)
    G, N = M.shape
    l = om.shape[1]
    host = gficf_amd.rsvd(M, k, q=q, omega=om, centre=centre)
    ops = HipOps(0)
    dev = torch.device("cuda", 0)
    cp, ri, xv = (torch.from_numpy(a).to(dev) for a in (M.indptr.astype(np.int64), M.indices.astype(np.int32), M.data))
    omd = torch.from_numpy(np.ascontiguousarray(om.T)).to(dev)
    d = torch.zeros(k, dtype=torch.float64, device=dev)
    cells = torch.zeros((k, N), dtype=torch.float64, device=dev)
    genes = torch.zeros((k, G), dtype=torch.float64, device=dev)
    mean = torch.zeros(G, dtype=torch.float64, device=dev)
    ws = torch.empty(ops.rsvd_workspace_bytes(G, N, M.nnz, l), dtype=torch.uint8, device=dev)
    ops.rsvd(G, N, cp, ri, xv, centre, omd, k, l, q, ws, d, cells, genes, mean)
    ops.rsvd_sync(ws)
    assert np.array_equal(d.cpu().numpy(), host["d"])
    assert np.array_equal(cells.cpu().numpy().T, host["cells"]) and np.array_equal(genes.cpu().numpy().T, host["v"])
    if centre:
        assert np.array_equal(mean.cpu().numpy(), host["centre"])


# ------------------------------------------------------------------------------------------------ blocks, rank < l
BLOCKS = {"cells_tall": (200, 100), "genes_tall": (200, 260)}
BLOCKS_MEASURED = {"cells_tall": {"d": 2.2e-15, "cells": 9.1e-16, "genes": 6.9e-16},
                   "genes_tall": {"d": 8.3e-16, "cells": 1.6e-16, "genes": 4.2e-16}}


def _blocks_input(name):
    N, G = BLOCKS[name]
    # d = a sqrt(n g): 3 sqrt(60 * 20), 2 sqrt(50 * 30), 1.5 sqrt(40 * 25), 1 sqrt(30 * 10) = 103.9, 77.5, 47.4, 17.3
    return rp.blocks(N, G, [60, 50, 40, 30], [20, 30, 25, 10], [3.0, 2.0, 1.5, 1.0]) + (_omega(min(N, G), 12, seed=23),)


@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_blocks_closed_form_at_rank_below_l(name):
    M, d, U, V, om = _blocks_input(name)
    got = gficf_amd.rsvd(M, 4, q=2, omega=om)
    for key in ("d", "cells", "v"):
        assert np.isfinite(got[key]).all()
    want = rp.rsvd(M, om, 4, 2, False, "lapack")
    dev = rp.deviations(want, {"d": got["d"], "cells": got["cells"], "genes": got["v"]})
    for key in ("d", "cells", "genes"):
        assert dev[key] <= rp.tolerance(BLOCKS_MEASURED[name][key]), (key, dev[key])
    # and the closed form, at the bound the port itself is held to (tests/test_pca_cpu.py)
    assert np.allclose(got["d"], d, rtol=1e-12, atol=0)
    assert np.allclose(got["v"], V, rtol=0, atol=1e-12) and np.allclose(got["cells"], U * d, rtol=0, atol=1e-12 * d[0])
    # the projection of the training cells is `cells`: A V = U d when the rank is k
    proj = gficf_amd.pca_project({"pca": {"genes": got["v"], "centre": False}}, M)
    assert np.abs(proj - got["cells"]).max() <= rp.tolerance(BLOCKS_MEASURED[name]["cells"]) * d[0]
    # all l = 12 values: the eight past the rank are dropped, not noise
    full = gficf_amd.rsvd(M, 12, q=2, omega=om)
    assert np.isfinite(full["cells"]).all() and np.isfinite(full["v"]).all()
    assert (full["d"][4:] == 0).all() and (full["v"][:, 4:] == 0).all() and (full["cells"][:, 4:] == 0).all()


# ------------------------------------------------------------------------------------------------ the projection
def test_pca_project_on_the_training_cells():
    M, om, k, q, _ = _rsvd_input("cells_tall_centre")
    data = gficf_amd.runPCA({"gficf": M}, dim=k, centre=True)
    genes, mu = data["pca"]["genes"], data["pca"]["mean"]
    got = gficf_amd.pca_project(data, M)
    want = M.T @ genes - (mu @ genes)[None, :]
    # per element: the column's n products and the correction's G, in any order
    n = np.diff(M.indptr)
    bound = _gamma(n + M.shape[0] + 2)[:, None] * (abs(M).T @ np.abs(genes) + (np.abs(mu) @ np.abs(genes))[None, :])
    assert (np.abs(got - want) <= bound).all()
    # without centring the means are not touched
    lsa = gficf_amd.runLSA({"gficf": M}, dim=k, centre=True)
    assert lsa["pca"]["centre"] is False and lsa["pca"]["mean"] is None
    got = gficf_amd.pca_project(lsa, M[:, :50])
    want = M[:, :50].T @ lsa["pca"]["genes"]
    assert (np.abs(got - want) <= _gamma(n[:50] + 2)[:, None] * (abs(M[:, :50]).T @ np.abs(lsa["pca"]["genes"]))).all()


# ------------------------------------------------------------------------------------------------ error codes
def _raises(status, fn):
    with pytest.raises(GficfError) as e:
        fn()
    assert e.value.status == status, (e.value.status, str(e.value))


def _usable():
    M, om, k, q, centre = _rsvd_input("k1")
    r = gficf_amd.rsvd(M, k, q=q, omega=om)
    assert np.isfinite(r["d"]).all() and r["d"][0] > 0


def test_error_codes_and_the_context_stays_usable():
    M, om, k, q, _ = _rsvd_input("cells_tall")
    G, N = M.shape
    bad = M.copy(); bad.data[17] = np.nan
    _raises("GFICF_ERR_BAD_VALUE", lambda: gficf_amd.rsvd(bad, k, omega=om))
    _usable()
    bad = M.copy(); bad.data[5] = np.inf
    _raises("GFICF_ERR_BAD_VALUE", lambda: gficf_amd.csc_tmm(bad, np.ones((G, 3))))
    _usable()
    omb = om.copy(); omb[3, 2] = np.nan
    _raises("GFICF_ERR_BAD_VALUE", lambda: gficf_amd.rsvd(M, k, omega=omb))
    _usable()
    for wrong in (G, -1):
        bad = sp.csc_matrix(M.copy())
        bad.indices[40] = wrong
        bad.has_sorted_indices = True
        _raises("GFICF_ERR_BAD_CSC", lambda: gficf_amd.rsvd(bad, k, omega=om))
        _usable()
        _raises("GFICF_ERR_BAD_CSC", lambda: gficf_amd.csc_tmm(bad, np.ones((G, 3))))
        _usable()
    bad = sp.csc_matrix(M.copy())
    bad.indptr[10] = bad.indptr[9] - 1
    bad.has_sorted_indices = True
    _raises("GFICF_ERR_BAD_CSC", lambda: gficf_amd.rsvd(bad, k, omega=om))
    _raises("GFICF_ERR_BAD_CSC", lambda: gficf_amd.csc_tmm(bad, np.ones((G, 3))))
    _usable()
    _raises("GFICF_ERR_INVALID_ARG", lambda: gficf_amd.rsvd(M, 0, omega=om))                       # k < 1
    _raises("GFICF_ERR_INVALID_ARG", lambda: gficf_amd.rsvd(M, om.shape[1] + 1, omega=om))         # k > l
    _raises("GFICF_ERR_INVALID_ARG", lambda: gficf_amd.rsvd(M, 5, omega=_omega(G, 129)))           # l > 128
    small = M[:20, :]
    _raises("GFICF_ERR_INVALID_ARG", lambda: gficf_amd.rsvd(small, 5, omega=_omega(20, 21)))       # l > min(N, G)
    _raises("GFICF_ERR_INVALID_ARG", lambda: gficf_amd.rsvd(M, 5, q=-1, omega=om))
    _raises("GFICF_ERR_INVALID_ARG", lambda: gficf_amd.csc_tmm(M, np.ones((G, 129))))
    _usable()


def test_device_form_deferred_errors_and_short_workspace():
    import torch

    M, om, k, q, _ = _rsvd_input("cells_tall")
    G, N = M.shape
    l = om.shape[1]
    ops = HipOps(0)
    dev = torch.device("cuda", 0)
    omd = torch.from_numpy(np.ascontiguousarray(om.T)).to(dev)
    d = torch.zeros(k, dtype=torch.float64, device=dev)
    cells = torch.zeros((k, N), dtype=torch.float64, device=dev)
    genes = torch.zeros((k, G), dtype=torch.float64, device=dev)
    need = ops.rsvd_workspace_bytes(G, N, M.nnz, l)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def run(indptr, indices, data, w=ws):
        cp, ri, xv = (torch.from_numpy(a).to(dev) for a in (indptr.astype(np.int64), indices.astype(np.int32), data))
        ops.rsvd(G, N, cp, ri, xv, False, omd, k, l, q, w, d, cells, genes)
        ops.rsvd_sync(w)

    _raises("GFICF_ERR_CAPACITY", lambda: run(M.indptr, M.indices, M.data, ws[: need - 4096]))
    ip = M.indptr.copy(); ip[10] = ip[9] - 1                                                       # not monotone, on the device
    _raises("GFICF_ERR_BAD_CSC", lambda: run(ip, M.indices, M.data))
    ix = M.indices.copy(); ix[40] = G
    _raises("GFICF_ERR_BAD_CSC", lambda: run(M.indptr, ix, M.data))
    xv = M.data.copy(); xv[3] = np.nan
    _raises("GFICF_ERR_BAD_VALUE", lambda: run(M.indptr, M.indices, xv))
    run(M.indptr, M.indices, M.data)                                                               # and the same context and workspace still work
    host = gficf_amd.rsvd(M, k, q=q, omega=om)
    assert np.array_equal(d.cpu().numpy(), host["d"]) and np.array_equal(genes.cpu().numpy().T, host["v"])
    # a short workspace of the other device entries
    Yd = torch.zeros((8, 100), dtype=torch.float64, device=dev)
    _raises("GFICF_ERR_CAPACITY", lambda: ops.orthonormalize(100, 8, Yd, ws[:256]))
    _raises("GFICF_ERR_INVALID_ARG", lambda: ops.orthonormalize(4, 8, Yd, ws))                     # fewer rows than columns


# ------------------------------------------------------------------------------------------------ end to end
E2E = dict(N=3000, C=6, G=1200, seed=31)


@pytest.fixture(scope="module")
def e2e():
    M, group = rp.planted_counts(**E2E)
    data = gficf_amd.gficf(M, verbose=False)
    return data, group


def test_end_to_end_gficf_runpca_clustcells(e2e):
    data, group = e2e
    data = gficf_amd.runPCA(dict(data), dim=10)
    assert data["dimPCA"] == 10 and data["pca"]["cells"].shape == (E2E["N"], 10) and data["pca"]["centre"] is False
    data = gficf_amd.clustcells(data, k=15, verbose=False)
    # every cell's 15 nearest neighbours in the returned PCA space belong to its group (checked on the CPU with the port
    # before the generator's settings were fixed)
    nn = gficf_amd.find_nn(data["pca"]["cells"], 16, True, "manhattan")["idx"][:, 1:] - 1
    assert (group[nn] == group[:, None]).all()
    # every community lies inside one planted group
    for c in np.unique(data["community"]):
        assert len(np.unique(group[data["community"] == c])) == 1, c


def test_runlsa_against_the_port():
    M, _, k, q, _ = _rsvd_input("cells_tall")
    G, N = M.shape
    lsa = gficf_amd.runLSA({"gficf": M}, dim=k, seed=22, centre=True)              # (centre is accepted and not used, as in the reference)
    assert lsa["pca"]["rescale"] is False and lsa["pca"]["centre"] is False and lsa["dimPCA"] == k
    om = np.random.default_rng(22).standard_normal((min(G, N), k + 10))            # what the mirror draws: p = 10
    want = rp.rsvd(M, om, k, 2, False, "lapack")
    cells = lsa["pca"]["cells"]
    _against_port({"d": np.linalg.norm(cells, axis=0), "cells": cells, "v": lsa["pca"]["genes"]}, want, RSVD_MEASURED["cells_tall"])
    pca = gficf_amd.runPCA({"gficf": M}, dim=k, seed=22)                           # rpca without centring is the same decomposition
    assert np.array_equal(pca["pca"]["cells"], cells) and np.array_equal(pca["pca"]["genes"], lsa["pca"]["genes"])


def test_computepcadim_returns_the_rule_on_the_ports_d(e2e, capsys):
    data, _ = e2e
    M = data["gficf"]
    G, N = M.shape
    om = np.random.default_rng(180582).standard_normal((min(G, N), 60))            # k = min(50, N), p = 10, the default seed
    rule = gficf_amd.pca_dim_rule(rp.rsvd(M, om, 50, 2, False, "lapack")["d"])
    assert rule is not None
    out = gficf_amd.computePCADim(dict(data))
    assert out["dimPCA"] == rule
    assert f"Number of estimated dimensions = {rule}" in capsys.readouterr().out
    assert gficf_amd.runPCA(out)["pca"]["cells"].shape == (N, rule)                # dim = None takes data["dimPCA"]
    sub = gficf_amd.computePCADim(dict(data), subsampling=True)                    # 5 % of the cells: 150, so k = 50, l = 60
    assert isinstance(sub["dimPCA"], int)


# ------------------------------------------------------------------------------------------------ config-3 scale
@pytest.fixture(scope="module")
def config3():
    G, N = 23000, 54000
    colptr, rowidx, x = synth.counts_csc(G, N)
    data = gficf_amd.gficf(sp.csc_matrix((x, rowidx, colptr), shape=(G, N)), storeRaw=False, verbose=False)
    return gficf_amd.runPCA(data, dim=50)


def test_config3_scale_properties(config3):
    data = config3
    M, cells, genes = data["gficf"], data["pca"]["cells"], data["pca"]["genes"]
    G, N = M.shape
    k, l = 50, 60
    assert cells.shape == (N, k) and genes.shape == (G, k)
    d = np.linalg.norm(cells, axis=0)
    assert (np.diff(d) <= 0).all() and d[-1] > 0
    # genes = B'W / d comes from ONE Gram matrix of B' (n x l): its columns are orthonormal up to eps * (d[0] / d[j])^2 per
    # unit of the l-term sums behind them, plus the gamma_m of the m-term dot products (the library's and this check's)
    tol = 64 * l * EPS * (d[0] / d[-1]) ** 2 + 4 * max(G, N) * EPS
    assert np.abs(genes.T @ genes - np.eye(k)).max() <= tol
    U = cells / d
    assert np.abs(U.T @ U - np.eye(k)).max() <= tol
    # A' cells = genes diag(d^2): an identity of the algorithm (A'Q W d = B'W d = V d^2), whatever the sketch's quality;
    # per element the m-term products of scipy's evaluation and of the library's, relative to d[0]^2
    lhs = M @ cells
    assert np.abs(lhs - genes * d ** 2).max() <= (tol + 4 * _gamma(N)) * d[0] ** 2
    again = gficf_amd.runPCA({"gficf": M}, dim=50)
    assert np.array_equal(again["pca"]["cells"], cells) and np.array_equal(again["pca"]["genes"], genes)


REDUCED_MEASURED = {"d": 3.5e-16}                                 # 8 000 genes x 20 000 cells, k = 50: d / d[0] between the port's variants


def test_reduced_size_d_against_the_port():
    G, N = 8000, 20000
    colptr, rowidx, x = synth.counts_csc(G, N)
    M = gficf_amd.gficf(sp.csc_matrix((x, rowidx, colptr), shape=(G, N)), storeRaw=False, verbose=False)["gficf"]
    om = _omega(min(M.shape), 60, seed=41)
    got = gficf_amd.rsvd(M, 50, omega=om)
    want = rp.rsvd(M, om, 50, 2, False, "lapack")
    assert np.abs(got["d"] - want["d"]).max() / want["d"][0] <= rp.tolerance(REDUCED_MEASURED["d"])
