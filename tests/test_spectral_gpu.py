"""GPU: libgficf_spectral.so (connected components, the Laplacian eigen-solve) and its Python mirror.

Components are compared to scipy's, relabelled to the smallest id, exactly.  The eigen-solve is held to defining properties and
to ``eigh`` of the dense operator (tests/helpers/spectral_np.py): no second copy of the block solver.

Where the tolerances come from.
  ring     theta against the closed form: 1e-12, a thousand roundings of the f64 sums (the eigenvalue error of a vector with
           residual r is r^2 / gap, far below that at tol = 1e-10).  The radius sqrt(2 / N) of every point in the returned plane:
           a CPU prototype of the method gave a relative spread of 2e-9 (N = 300) and 3e-10 (N = 64); 100 x that for a different
           summation order.
  angles   Davis-Kahan: sin <= residual / gap, the residual recomputed on the host, the gap from the dense spectrum.
  the rest |S x - theta x| <= tol |theta| + 1e-12 (the contract), |V' q0| and |V' V - I| <= 1e-10 (two projection passes in f64).
Quality.  Trustworthiness and 15-NN label purity of umap(init="spectral") on the connected blobs against the numpy port's own
figures from the start array ``eigh`` gives (PORT_QUALITY; ``python -m tests.helpers.spectral_np`` recomputes them), by the rule
of tests/test_umap_gpu.py: no more than 0.01 below the port's worst seed."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import gficf_amd
from gficf_amd import GficfError
from gficf_amd.api import HipOps, umap_init
from tests.helpers import spectral_cases as sc
from tests.helpers import spectral_np as sn
from tests.helpers import umap_cases as uc
from tests.helpers import umap_np as un

pytestmark = pytest.mark.gpu

# (trustworthiness, purity) of the port from eigh's start, seeds 1 - 5, 200 epochs, un.blobs(1200, 12, 20, 1.0, 0)
PORT_QUALITY = [(0.95593, 0.9715), (0.95517, 0.97028), (0.95562, 0.97117), (0.95566, 0.96983), (0.95566, 0.96578)]
RING_SPREAD = {300: 100 * 2e-9, 64: 100 * 3e-10}


def _graph_of(X, k=15):
    r = gficf_amd.find_nn(X, k, True, "euclidean")
    return gficf_amd.fuzzy_simplicial_set(r["idx"], r["dist"])[0]


@pytest.fixture(scope="module")
def blobs12():
    """un.blobs(1200, 12, 20, 3.0, 0) at k = 15: the project's usual blob fixture, 12 components."""
    X, _ = un.blobs(1200, 12, 20, 3.0, 0)
    return X, _graph_of(X)


@pytest.fixture(scope="module")
def connected():
    """Case 2: (X, labels, P, values, vectors, q0) of the connected blobs; the spectrum by eigh, once."""
    X, labels, _, _ = sn.connected_blobs()
    P = _graph_of(X)
    w, U, q0 = sn.spectrum(P)
    return X, labels, P, w, U, q0


# ------------------------------------------------------------------------------------------------ components
def _sym(i, j, N):
    v = np.ones(2 * len(i), np.float32)
    P = sp.csr_matrix((v, (np.concatenate([i, j]), np.concatenate([j, i]))), shape=(N, N))
    P.sum_duplicates()
    P.sort_indices()
    return P


def _component_cases():
    rng = np.random.default_rng(3)
    perm = rng.permutation(4096)
    cases = {"path": _sym(perm[:-1], perm[1:], 4096)}
    cases["rings"] = sp.block_diag([sn.ring(50, 1), sp.csr_matrix((1, 1), dtype=np.float32), sn.ring(31, 2)], format="csr")
    centre = 1500
    others = np.delete(np.arange(3001), centre)
    cases["star"] = _sym(np.full(3000, centre), others, 3001)
    i, j = rng.integers(0, 400, 300), rng.integers(0, 400, 300)
    keep = i < j
    cases["upper"] = sp.csr_matrix((np.ones(keep.sum(), np.float32), (i[keep], j[keep])), shape=(400, 400))
    return cases


COMPONENT_CASES = _component_cases()


@pytest.mark.parametrize("name", list(COMPONENT_CASES))
def test_components_match_scipy_exactly(name):
    P = COMPONENT_CASES[name]
    want, n = sn.components(P)
    got, m, rounds = gficf_amd.graph_components(P, ret_rounds=True)
    print(f"{name}: {m} components in {rounds} rounds")
    assert got.dtype == np.int32 and m == n and np.array_equal(got, want)
    assert 1 <= rounds <= 128                        # a condition: a min-label sweep needs about 4 096 rounds on the path
    if name == "path":
        assert n == 1
    if name == "rings":
        assert n == 3 and got[50] == 50
    if name == "star":
        assert np.diff(P.indptr).max() == 3000 and n == 1
    if name == "upper":
        assert (P != P.T).nnz > 0 and n > 1
    assert np.array_equal(gficf_amd.graph_components(P)[0], got)


def test_components_of_the_blob_graph(blobs12):
    _, P = blobs12
    want, n = sn.components(P)
    got, m = gficf_amd.graph_components(P)
    assert n == 12 and m == 12 and np.array_equal(got, want)


def test_components_refuse_bad_rows_and_columns():
    import torch

    ops = HipOps(0)
    P = sn.ring(10, 1)

    def run(indptr, indices):
        rowptr = torch.from_numpy(np.asarray(indptr, np.int64)).cuda()
        col = torch.from_numpy(np.asarray(indices, np.int32)).cuda()
        labels = torch.full((10,), -7, dtype=torch.int32, device="cuda")
        info = torch.zeros(2, dtype=torch.int64, device="cuda")
        ws = torch.empty(ops.graph_components_workspace_bytes(10), dtype=torch.uint8, device="cuda")
        ops.graph_components(10, rowptr, col, len(indices), labels, info, ws)
        return int(info[0].item())

    assert run(P.indptr, P.indices) == 1
    for bad in (10, -1, 2 ** 31 - 1):
        ind = P.indices.copy()
        ind[7] = bad
        with pytest.raises(GficfError) as e:
            run(P.indptr, ind)
        assert e.value.status == "GFICF_ERR_BAD_ID"
    for at, v in ((4, 2), (10, 21), (0, 1)):                   # decreasing, past the capacity, not starting at 0
        ptr = P.indptr.astype(np.int64).copy()
        ptr[at] = v
        with pytest.raises(GficfError) as e:
            run(ptr, P.indices)
        assert e.value.status == "GFICF_ERR_BAD_CSC"
    assert run(P.indptr, P.indices) == 1                        # the context is still good


# ------------------------------------------------------------------------------------------------ the properties every solve is held to
_check_solution = sc.check_solution                            # shared with tests/test_spectral_ndim_gpu.py and the CPU tests


# ------------------------------------------------------------------------------------------------ 1. the ring
@pytest.mark.parametrize("N,s", [(300, 3), (64, 2)])
def test_ring_returns_the_degenerate_plane(N, s):
    P = sn.ring(N, s)
    r = gficf_amd.spectral_embedding(P, 2, tol=1e-10, seed=1)
    _check_solution(P, r, 1e-10)
    want = sn.ring_value(N, s)
    radius = np.sqrt((r["vectors"] ** 2).sum(axis=1))
    spread = float(np.abs(radius / np.sqrt(2.0 / N) - 1.0).max())
    print(f"ring {N}: theta - closed form {r['values'] - want}, relative radius spread {spread:.3e} (allowed {RING_SPREAD[N]:.1e})")
    assert np.abs(r["values"] - want).max() <= 1e-12                                # BOTH: a single-vector solver returns the next plane second
    assert spread <= RING_SPREAD[N]


# ------------------------------------------------------------------------------------------------ 2. connected blobs, 3. the hub row
def _against_eigh(P, r, w, U, q0, tol):
    res = _check_solution(P, r, tol, w, q0)
    for l in range(r["vectors"].shape[1]):
        assert abs(r["values"][l] - w[1 + l]) <= tol
        bound = sn.davis_kahan(w, 1 + l, res[l])
        got = sn.sine(r["vectors"][:, l], U[:, 1 + l])
        print(f"vector {l}: sine to eigh's {got:.3e}, Davis-Kahan bound {bound:.3e}")
        assert got <= bound * (1 + 1e-6) + 1e-12


def test_connected_blobs_against_eigh(connected):
    _, _, P, w, U, q0 = connected
    assert sn.components(P)[1] == 1 and np.allclose(w[:4], [1.0, 0.984967, 0.981334, 0.978760], atol=2e-6)
    r = gficf_amd.spectral_embedding(P)
    _against_eigh(P, r, w, U, q0, 1e-4)


def test_hub_row_graph():
    P, _ = uc.layout_graph("hub")
    assert P.shape == (2001, 2001) and np.diff(P.indptr).max() == 2000 and gficf_amd.graph_components(P)[1] == 1
    w, U, q0 = sn.spectrum(P)
    r = gficf_amd.spectral_embedding(P)
    _against_eigh(P, r, w, U, q0, 1e-4)


# ------------------------------------------------------------------------------------------------ 4. small N
@pytest.mark.parametrize("kind,N", [(k, n) for k in ("ring", "complete") for n in (4, 5, 6, 33)])
def test_small_graphs(kind, N):
    P = sn.ring(N, 1) if kind == "ring" else sn.complete(N)
    w, U, q0 = sn.spectrum(P)
    r = gficf_amd.spectral_embedding(P, 2, seed=N)
    _check_solution(P, r, 1e-4, w, q0)
    assert r["restarts"] == 0                                   # the basis, capped at N - 1 columns, spans the whole complement
    assert np.abs(r["values"] - w[1:3]).max() <= 1e-12
    cluster = U[:, (np.abs(w[:, None] - r["values"][None, :]) <= 1e-9).any(axis=1)]        # every eigenvector of a returned value
    assert cluster.shape[1] >= 2 and np.abs(cluster.T @ q0).max() < 1e-9
    off = np.linalg.norm(r["vectors"] - cluster @ (cluster.T @ r["vectors"]), axis=0)
    print(f"{kind} {N}: {cluster.shape[1]} eigenvectors share the returned values; outside their span {off}")
    assert off.max() <= 1e-10


# ------------------------------------------------------------------------------------------------ 5. disconnected
def test_disconnected_graph_is_reported_not_solved(blobs12):
    import torch

    X, P = blobs12
    with pytest.raises(ValueError, match="12"):
        gficf_amd.spectral_embedding(P)
    with pytest.raises(ValueError, match="12"):
        gficf_amd.spectral_init(P)
    ops = HipOps(0)
    N, cap = P.shape[0], P.nnz
    rowptr = torch.from_numpy(P.indptr.astype(np.int64)).cuda()
    col = torch.from_numpy(P.indices.astype(np.int32)).cuda()
    val = torch.from_numpy(P.data.astype(np.float32)).cuda()
    start = torch.from_numpy(np.random.default_rng(0).standard_normal((N, 2))).cuda()
    theta, resid = torch.full((2,), 777.0, dtype=torch.float64, device="cuda"), torch.full((2,), 777.0, dtype=torch.float64, device="cuda")
    vectors = torch.full((N, 2), 777.0, dtype=torch.float64, device="cuda")
    info = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    ws = torch.empty(ops.spectral_workspace_bytes(N, cap, 2, 32), dtype=torch.uint8, device="cuda")
    ops.spectral(N, rowptr, col, val, cap, 2, start, 1e-4, 32, 200, ws, theta, resid, vectors, info)
    assert info.cpu().tolist() == [12, 0, 0, 0]
    assert (vectors == 777.0).all().item() and (theta == 777.0).all().item() and (resid == 777.0).all().item()


def test_umap_spectral_on_a_disconnected_graph_starts_from_pca(blobs12):
    X, _ = blobs12
    with pytest.warns(UserWarning, match="12"):
        got = gficf_amd.umap(X, "spectral", n_epochs=30, seed=7)
    want = gficf_amd.umap(X, umap_init("pca", X, len(X), 7), n_epochs=30, seed=7)
    assert np.array_equal(got["embedding"], want["embedding"])
    assert (got["graph"] != want["graph"]).nnz == 0 and np.array_equal(got["nn"]["idx"], want["nn"]["idx"])
    assert set(got) == set(want) and all(got[k] == want[k] for k in ("a", "b", "n_neighbors", "metric", "n_epochs", "seed"))


def test_host_entry_equals_the_device_entry(connected, blobs12):
    """gficf_spectral_host: components first, the solve only for one component; the bits of the device entry."""
    from gficf_amd import _spectral_lib
    from gficf_amd._lib import check
    from gficf_amd.api import _np_ptr

    L, ctx = _spectral_lib.load(), gficf_amd.default_context()
    for P, n_comp in ((connected[2], 1), (blobs12[1], 12)):
        N = P.shape[0]
        start = np.random.default_rng(21).standard_normal((N, 2))
        rowptr, col, val = P.indptr.astype(np.int64), P.indices.astype(np.int32), P.data.astype(np.float32)
        labels, info = np.full(N, -1, np.int32), np.full(4, -1, np.int64)
        theta, resid, vectors = np.full(2, 777.0), np.full(2, 777.0), np.full((N, 2), 777.0)
        check(L.gficf_spectral_host(ctx.handle, N, _np_ptr(rowptr), _np_ptr(col), _np_ptr(val), 2, _np_ptr(start), 1e-4, 32, 200, _np_ptr(labels),
                                    _np_ptr(theta), _np_ptr(resid), _np_ptr(vectors), _np_ptr(info)))
        assert np.array_equal(labels, sn.components(P)[0]) and info[0] == n_comp
        if n_comp == 1:
            r = gficf_amd.spectral_embedding(P, start=start)
            assert np.array_equal(vectors, r["vectors"]) and np.array_equal(theta, r["values"]) and np.array_equal(resid, r["residuals"])
            assert info.tolist() == [1, r["restarts"], r["multiplications"], 1]
        else:
            assert info.tolist() == [12, 0, 0, 0] and (vectors == 777.0).all() and (theta == 777.0).all() and (resid == 777.0).all()
    bad = connected[2].indices.astype(np.int32).copy()
    bad[5] = N + 3
    P = connected[2]
    with pytest.raises(GficfError) as e:
        check(L.gficf_spectral_host(ctx.handle, P.shape[0], _np_ptr(P.indptr.astype(np.int64)), _np_ptr(bad), _np_ptr(P.data.astype(np.float32)), 2,
                                    _np_ptr(start), 1e-4, 32, 200, None, _np_ptr(theta), _np_ptr(resid), _np_ptr(vectors), _np_ptr(info)))
    assert e.value.status == "GFICF_ERR_BAD_ID"
    val = P.data.astype(np.float32).copy()
    val[3] = -1.0
    with pytest.raises(GficfError) as e:
        check(L.gficf_spectral_host(ctx.handle, P.shape[0], _np_ptr(P.indptr.astype(np.int64)), _np_ptr(P.indices.astype(np.int32)), _np_ptr(val), 2,
                                    _np_ptr(start), 1e-4, 32, 200, None, _np_ptr(theta), _np_ptr(resid), _np_ptr(vectors), _np_ptr(info)))
    assert e.value.status == "GFICF_ERR_BAD_VALUE"
    with pytest.raises(GficfError) as e:
        check(L.gficf_spectral_host(ctx.handle, P.shape[0], _np_ptr(P.indptr.astype(np.int64)), _np_ptr(P.indices.astype(np.int32)), _np_ptr(val), 9,
                                    _np_ptr(start), 1e-4, 32, 200, None, _np_ptr(theta), _np_ptr(resid), _np_ptr(vectors), _np_ptr(info)))
    assert e.value.status == "GFICF_ERR_INVALID_ARG"


# ------------------------------------------------------------------------------------------------ 6. determinism
def test_same_bits_and_start_blocks_agree(connected):
    _, _, P, w, U, _ = connected
    a = gficf_amd.spectral_embedding(P, seed=11)
    b = gficf_amd.spectral_embedding(P, seed=11)
    assert np.array_equal(a["vectors"], b["vectors"]) and np.array_equal(a["values"], b["values"]) and np.array_equal(a["residuals"], b["residuals"])
    c = gficf_amd.spectral_embedding(P, start=np.random.default_rng(12).uniform(-1, 1, size=(P.shape[0], 2)))
    assert not np.array_equal(a["vectors"], c["vectors"])
    for l in range(2):
        bound = sn.davis_kahan(w, 1 + l, a["residuals"][l]) + sn.davis_kahan(w, 1 + l, c["residuals"][l])
        got = sn.sine(a["vectors"][:, l], c["vectors"][:, l])
        print(f"vector {l}: sine between the two starts {got:.3e}, bound {bound:.3e}")
        assert got <= bound * (1 + 1e-6) + 1e-12 and a["vectors"][:, l] @ c["vectors"][:, l] > 0       # the sign rule made them agree


# ------------------------------------------------------------------------------------------------ 7. not converged
def test_no_restarts_returns_what_it_has():
    P = sn.ring(300, 3)
    with pytest.warns(UserWarning, match="not converged"):
        r = gficf_amd.spectral_embedding(P, 2, tol=1e-10, max_restarts=0, seed=1)
    assert not r["converged"] and r["restarts"] == 0 and r["n_components"] == 1
    assert np.isfinite(r["vectors"]).all() and np.allclose(np.linalg.norm(r["vectors"], axis=0), 1.0, atol=1e-12)
    res = sn.residuals(P, r["vectors"], r["values"])
    assert (res > 1e-10 * np.abs(r["values"])).any() and np.allclose(r["residuals"], res, rtol=1e-6, atol=1e-14)     # truthful


# ------------------------------------------------------------------------------------------------ 8. spectral_init and the embedding from it
def test_spectral_init_scaling_and_noise(connected):
    _, _, P, w, U, _ = connected
    Y = gficf_amd.spectral_init(P, seed=5)
    raw = gficf_amd.spectral_init(P, seed=5, jitter=False)
    assert Y.shape == (1200, 2) and Y.dtype == np.float64 and abs(np.abs(Y).max() - 10.0) < 1e-3
    assert np.allclose(np.linalg.norm(raw, axis=0), 1.0, atol=1e-12)
    rng = np.random.default_rng(5)
    rng.standard_normal((1200, 2))                                                  # the start block is drawn first
    assert np.allclose(Y - raw * (10.0 / np.abs(raw).max()), rng.normal(0.0, 1e-4, size=(1200, 2)), rtol=0, atol=1e-12)
    assert np.array_equal(gficf_amd.spectral_init(P, seed=5), Y)


def test_run_reduction_normlaplacian(connected):
    X = connected[0]
    data = gficf_amd.runReduction({"pca": {"cells": X}}, init="normlaplacian", n_epochs=20, seed=3, verbose=False)
    want = gficf_amd.umap(X, "normlaplacian", n_epochs=20, seed=3)
    assert np.array_equal(np.asarray(data["embedded"]), want["embedding"]) and np.isfinite(want["embedding"]).all()


def test_quality_of_the_spectral_start(connected):
    X, labels, P, _, _, _ = connected
    port_trust, port_purity = min(t for t, _ in PORT_QUALITY), min(p for _, p in PORT_QUALITY)
    for seed in sn.QUALITY_SEEDS:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            r = gficf_amd.umap(X, "spectral", n_epochs=sn.QUALITY_EPOCHS, seed=seed)
        assert not [c for c in caught if "component" in str(c.message) or "converged" in str(c.message)]      # connected and converged
        trust, purity = un.quality(X, r["embedding"], labels)
        print(f"seed {seed}: trustworthiness {trust:.5f} (port at least {port_trust:.5f}), purity {purity:.5f} (port at least {port_purity:.5f})")
        assert np.isfinite(r["embedding"]).all()
        assert trust >= port_trust - 0.01
        assert purity >= port_purity - 0.01
