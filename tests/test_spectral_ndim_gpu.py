"""GPU: the eigen-solve of libgficf_spectral.so at every block width ndim = 1 .. 8 and at basis sizes m other than 32.

tests/test_spectral_gpu.py runs the solve at ndim = 2, m = 32 alone.  Here: every instantiation behind SP_DISPATCH, both bodies of
sp_row (even and odd b), every output chunk of k_sp_proj_part ((nc + 1) b = 264 at ndim 8, m 32 and 520 at m 64), the strided
hub loop (planted(): 1 100 hub rows for 1 024 waves), rows of exactly 256 and of 257 entries (threshold()), and the cycle's end:
at its last full block when the basis is capped by m, at the narrower block when it is capped by N - 1 (the small graphs).

Every solve is held to the properties of tests/helpers/spectral_cases.py (check_solution, unchanged from
tests/test_spectral_gpu.py) and to ``eigh`` of the dense operator, computed once per graph:
  values    |theta_l - w_{1 + l}| <= tol: the eigenvalue error of a vector with residual r <= tol |theta| is at most r.
  vectors   a gap after the last value asked for: the sine between the subspaces <= |residuals|_2 / sep (Davis-Kahan, sn.subspace_bound);
            ndim splits a degenerate eigenvalue (rings at odd ndim, the complete graphs): each vector's part outside the eigenvectors
            within 1e-9 of its value <= residual / delta (sn.outside_cluster).  Both with the slack 1e-6 relative + 1e-12 of
            tests/test_spectral_gpu.py for the rounding of the host's own products.
  restarts  at most 2 x those of the numpy statement of the method (tests/helpers/spectral_block_np.py) on the same start block,
            tol and m, plus 2: a Ritz estimate that rounding puts on the other side of tol moves the stop by a cycle or two, a
            stall costs tens of cycles.  Measured against the port, never against the device.

m = 2 ndim + 2 leaves room for one block per restarted cycle; there the header keeps the Ritz vectors that carry the previous
step (59, 70, 45 and 41 restarts of the numpy statement at ndim 2, 3, 5, 8 where the next Ritz pairs would take 276, 306, 193, 119)."""
import numpy as np
import pytest

import gficf_amd
from gficf_amd import GficfError
from gficf_amd.api import _spectral_solve
from tests.helpers import spectral_block_np as sb
from tests.helpers import spectral_cases as sc
from tests.helpers import spectral_np as sn

pytestmark = pytest.mark.gpu


def _solve(name, ndim, m, tol, start=None):
    P = sc.graph(name)[0]
    if start is None:
        start = sc.start_block(P.shape[0], ndim)
    return _spectral_solve(P, ndim, start=start, tol=tol, m=m, max_restarts=sc.MAX_RESTARTS)


def _counts(label, r, port):
    print(f"COUNTS {label}: device {r['restarts']} restarts {r['multiplications']} multiplications, "
          f"port {port['restarts']} restarts {port['multiplications']} multiplications")


@pytest.mark.parametrize("case", sc.MATRIX, ids=sc.case_id)
def test_every_block_width(case):
    name, ndim, m, tol = case
    r = _solve(name, ndim, m, tol)
    port = sc.port(name, ndim, m, tol)
    _counts(sc.case_id(case), r, port)
    sc.check_against_eigh(name, r, tol)
    if name == "ring-300-3":
        want = [sn.ring_value(300, 3, 1 + l // 2) for l in range(ndim)]
        assert np.abs(r["values"] - want).max() <= 1e-12
    assert r["restarts"] <= 2 * port["restarts"] + 2


@pytest.mark.parametrize("case", sc.SMALL, ids=sc.case_id)
def test_small_graphs_keep_the_narrower_block(case):
    """mc = N - 1: the basis spans the whole complement of q0 after one cycle, whose last block is as narrow as it has to be."""
    name, ndim, m, tol = case
    r = _solve(name, ndim, m, tol)
    sc.check_against_eigh(name, r, tol)
    assert r["restarts"] == 0 and sc.port(name, ndim, m, tol)["restarts"] == 0
    assert np.abs(r["values"] - sc.graph(name)[1][1:1 + ndim]).max() <= 1e-12


# ------------------------------------------------------------------------------------------------ start blocks that lose a column, or all
@pytest.mark.parametrize("ndim", [2, 3])
def test_duplicated_start_column_stays_dropped(ndim):
    P = sc.graph("blobs")[0]
    g, h = np.random.default_rng(7).standard_normal((2, P.shape[0]))
    start = np.stack([g, g, h][:ndim], axis=1)
    r = _solve("blobs", ndim, 32, 1e-4, start)
    port = sc.as_result(sb.solve(P, ndim, start, 1e-4, 32, sc.MAX_RESTARTS))
    _counts(f"duplicated-ndim{ndim}", r, port)
    sc.check_against_eigh("blobs", port, 1e-4)
    sc.check_against_eigh("blobs", r, 1e-4)
    assert r["restarts"] <= 2 * port["restarts"] + 2


def test_start_block_inside_the_trivial_eigenvector_is_refused():
    P, _, _, q0, _ = sc.graph("blobs")
    with pytest.raises(GficfError) as e:
        gficf_amd.spectral_embedding(P, 2, start=np.stack([q0, -3.0 * q0], axis=1))
    assert e.value.status == "GFICF_ERR_BAD_VALUE" and "spans 0 directions" in str(e.value)
    sc.check_against_eigh("blobs", _solve("blobs", 3, 32, 1e-4), 1e-4)                                # the context is still good


# ------------------------------------------------------------------------------------------------ determinism, the host entry
@pytest.mark.parametrize("ndim,m", [(5, 33), (8, 64)])
def test_same_bits_twice(ndim, m):
    a, b = _solve("blobs", ndim, m, 1e-4), _solve("blobs", ndim, m, 1e-4)
    assert a["converged"] and a["restarts"] == b["restarts"] and a["multiplications"] == b["multiplications"]
    assert np.array_equal(a["vectors"], b["vectors"]) and np.array_equal(a["values"], b["values"]) and np.array_equal(a["residuals"], b["residuals"])


def test_host_entry_equals_the_device_entry_at_ndim_3():
    from gficf_amd import _spectral_lib
    from gficf_amd._lib import check
    from gficf_amd.api import _np_ptr

    L, ctx = _spectral_lib.load(), gficf_amd.default_context()
    P = sc.graph("blobs")[0]
    N = P.shape[0]
    start = sc.start_block(N, 3)
    rowptr, col, val = P.indptr.astype(np.int64), P.indices.astype(np.int32), P.data.astype(np.float32)
    labels, info = np.full(N, -1, np.int32), np.full(4, -1, np.int64)
    theta, resid, vectors = np.full(3, 777.0), np.full(3, 777.0), np.full((N, 3), 777.0)
    check(L.gficf_spectral_host(ctx.handle, N, _np_ptr(rowptr), _np_ptr(col), _np_ptr(val), 3, _np_ptr(start), 1e-4, 32, 200, _np_ptr(labels),
                                _np_ptr(theta), _np_ptr(resid), _np_ptr(vectors), _np_ptr(info)))
    r = gficf_amd.spectral_embedding(P, 3, start=start)
    assert (labels == 0).all() and info.tolist() == [1, r["restarts"], r["multiplications"], 1]
    assert np.array_equal(vectors, r["vectors"]) and np.array_equal(theta, r["values"]) and np.array_equal(resid, r["residuals"])
