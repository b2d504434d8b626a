"""GPU: libgficf_svds.so at every block width b of its contract (1 .. 32), at the tightest basis m = k + 2 b and the widest
m = 128, with more than 64 vectors kept across a restart, with five chunks of rows, with a block that narrows, and on the
smallest matrices there are (tests/helpers/svds_cases.py; DESIGN.md, "svds at every width").  tests/test_svds_gpu.py runs b = 8
only, where the pitch of a block is its width, lanes 8 .. 31 of the projection multiply zeros and no restart keeps more than 64
vectors.

Accuracy is held to LAPACK by the rule of tests/test_svds_gpu.py (32 x the port's own figure, never below 64 eps); for the
vectors, where it is larger, to what the stopping criterion itself promises (svds_cases.vector_bound), because the port and
the device may stop a cycle apart.  Full reorthogonalisation lets the method heal a projection that is slightly wrong at the
price of cycles, so the work is held to the port's as well, and one cycle alone, where nothing heals, is compared with the
port's one cycle.  Every figure is printed before it is asserted."""
import warnings

import numpy as np
import pytest

import gficf_amd
from gficf_amd import GficfError
from gficf_amd.api import HipOps
from tests.helpers import rsvd_np as rp
from tests.helpers import svds_cases as sc
from tests.helpers import svds_np as sn

pytestmark = pytest.mark.gpu

EPS, TOL = sc.EPS, sc.TOL
_cache: dict = {}


def _solve(c, **kw):
    r = gficf_amd.svds(sc.matrix(c.matrix), c.k, centre=c.centre, tol=TOL, m=c.m, start=sc.start_of(c), **kw)
    r["genes"] = r["v"]
    return r


def _case(c):
    """(M, LAPACK, port, device), computed once."""
    if c not in _cache:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got = sc._freeze(_solve(c))
        _cache[c] = (sc.matrix(c.matrix), sc.lapack(c.matrix, c.k, c.centre), sc.port(c), got)
    return _cache[c]


def _work(r):
    return {q: r[q] for q in ("cycles", "products", "converged", "exhausted")}


# ------------------------------------------------------------------------------------------------ a. accuracy
@pytest.mark.parametrize("case", sc.ALL, ids=sc.case_id)
def test_device_matches_lapack_at_every_width(case):
    M, want, port, got = _case(case)
    fp, fg = sc._figures(want, port), sc._figures(want, got)
    vb = sc.vector_bound(case)
    allowed = {q: rp.tolerance(fp[q]) if q == "d" else max(rp.tolerance(fp[q]), vb) for q in fp}
    which = {q: "rule" if allowed[q] == rp.tolerance(fp[q]) else "criterion" for q in fp}
    print(sc.case_id(case), "port", fp, "device", fg, "allowed", allowed, "bound", which, "work device", _work(got), "port", _work(port))
    for q in fp:
        assert fg[q] <= allowed[q], (sc.case_id(case), q, fg[q], fp[q], allowed[q], which[q])
    assert got["cells"].shape == (M.shape[1], case.k) and got["genes"].shape == (M.shape[0], case.k)
    if case.centre:
        assert np.allclose(got["centre"], M.toarray().mean(axis=1), rtol=1e-13, atol=0)
    else:
        assert got["centre"] is None


# ------------------------------------------------------------------------------------------------ b. properties, the direct residual
@pytest.mark.parametrize("case", sc.ALL, ids=sc.case_id)
def test_properties_at_every_width(case):
    M, want, port, got = _case(case)
    sc.check_properties(sc.case_id(case), M, case.centre, case.k, port, got)


@pytest.mark.parametrize("case", sc.ALL, ids=sc.case_id)
def test_direct_residual_at_every_width(case):
    M, want, port, got = _case(case)
    sc.check_direct_residual(sc.case_id(case), M, case.centre, port, got)


# ------------------------------------------------------------------------------------------------ c. work
@pytest.mark.parametrize("case", sc.ALL, ids=sc.case_id)
def test_work_stays_within_twice_the_ports(case):
    """A Ritz estimate that rounding puts on the other side of tol moves the stop by a cycle; a projection that is wrong and
    healed by the reorthogonalisation costs tens (the rule of tests/test_spectral_ndim_gpu.py)."""
    M, want, port, got = _case(case)
    steps = sc.steps_of_one_cycle(case)
    print(sc.case_id(case), "device", _work(got), "port", _work(port), "steps of a full cycle", steps)
    assert got["converged"] == case.k or got["exhausted"]
    assert got["cycles"] <= 2 * port["cycles"] + 2
    assert got["products"] <= 2 * port["products"] + 2 * steps
    if case.group in ("NARROW", "TINY"):
        assert port["exhausted"] and port["cycles"] == 1
        assert got["exhausted"] == port["exhausted"] and got["cycles"] == 1 and got["products"] == port["products"]
        rank = int((want["d_all"] > 1e-9 * want["d_all"][0]).sum())
        assert (port["d"][rank:] == 0).all()
        assert (got["d"][rank:] == 0).all() and (got["genes"][:, rank:] == 0).all() and (got["cells"][:, rank:] == 0).all()
        assert (got["d"][:rank] > 0).all()


# ------------------------------------------------------------------------------------------------ d. one cycle, where nothing can heal
def _one_cycle_case(b):
    return sc.Case("ONE", "flat", 10, b, max(40, 10 + 2 * b), False)


@pytest.mark.parametrize("b", sc.ONE_CYCLE_B)
def test_one_cycle_is_the_ports_one_cycle(b):
    c = _one_cycle_case(b)
    M = sc.matrix(c.matrix)
    p1 = sc.port(c, 1)
    with pytest.warns(UserWarning, match=r"only \d+ of the 10 singular values converged"):
        r = _solve(c, max_cycles=1)
    open_pairs = p1["residuals"] > 1e-6
    dd = float(np.abs(r["d"] - p1["d"]).max() / p1["d"][0])
    with np.errstate(divide="ignore", invalid="ignore"):
        rr = np.abs(r["residuals"] - p1["residuals"]) / p1["residuals"]
    print("b", b, "m", c.m, "device", _work(r), "port", _work(p1), "d off", dd, "residuals off (relative)", rr.tolist(), "compared", open_pairs.tolist())
    assert r["cycles"] == 1 and not r["exhausted"]
    assert r["products"] == sn.schedule(0, min(M.shape), b, c.m) == p1["products"]
    assert r["converged"] == p1["converged"]
    assert dd <= 64 * EPS
    assert open_pairs.any()
    assert np.allclose(r["residuals"][open_pairs], p1["residuals"][open_pairs], rtol=1e-6, atol=1e-14)
    assert np.isfinite(r["cells"]).all() and np.isfinite(r["v"]).all() and np.isfinite(r["residuals"]).all()


@pytest.mark.parametrize("b", [5, 17, 32])
def test_device_form_gives_the_host_forms_bits(b):
    c = sc.Case("WIDTHS", "planted", 10, b, 128, False)
    M, want, port, got = _case(c)
    dev = sc._device_form(M, c.k, b, c.m, c.centre, sc.start_of(c))
    assert np.array_equal(dev["d"], got["d"]) and np.array_equal(dev["cells"], got["cells"]) and np.array_equal(dev["genes"], got["genes"])
    assert np.array_equal(dev["residuals"], got["residuals"])
    assert list(dev["info"]) == [got["cycles"], got["products"], got["converged"], int(got["exhausted"])]


@pytest.mark.parametrize("b", [1, 31])
def test_same_bits_twice(b):
    c = sc.Case("WIDTHS", "planted", 10, b, 10 + 2 * b, False)
    M, want, port, got = _case(c)
    again = _solve(c)
    for q in ("d", "cells", "v", "residuals"):
        assert np.array_equal(again[q], got[q]), q
    assert _work(again) == _work(got)


# ------------------------------------------------------------------------------------------------ e. argument edges
def _raises(status, fn):
    with pytest.raises(GficfError) as e:
        fn()
    assert e.value.status == status, (e.value.status, str(e.value))


def test_widths_outside_the_contract_are_refused_and_the_context_stays_usable():
    c = sc.Case("WIDTHS", "planted", 10, 5, 20, False)
    M, want, port, got = _case(c)
    G, N = M.shape
    n = min(G, N)
    # (k, b, m): b = 33; b = 0, a start with no column; b > m; k + 2 b = m + 1 with m < n
    for k, b, m in ((10, 33, 128), (10, 0, 40), (4, 8, 7), (10, 5, 19), (10, 32, 73)):
        assert m < n and not sn.check_args(n, k, b, m)
        assert HipOps.svds_workspace_bytes(G, N, M.nnz, k, b, m) == 0, (k, b, m)
        _raises("GFICF_ERR_INVALID_ARG", lambda: gficf_amd.svds(M, k, m=m, start=sc._start(n, b)))
    r = _solve(c)
    assert np.array_equal(r["d"], got["d"]) and np.array_equal(r["cells"], got["cells"])
