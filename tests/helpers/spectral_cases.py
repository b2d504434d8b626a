"""What tests/test_spectral_gpu.py, tests/test_spectral_ndim_gpu.py and tests/test_spectral_cpu.py share: the properties every
eigen-solve is held to, the checks against ``eigh`` of the dense operator, and the matrix of (graph, ndim, m, tol) at which the
solve is run at every block width.  The same checks are put to the device and to the numpy statement of the method
(tests/helpers/spectral_block_np.py): the latter proves that a case is solvable by the method and sets the restarts allowed."""
import functools

import numpy as np

from tests.helpers import spectral_block_np as sb
from tests.helpers import spectral_np as sn
from tests.helpers import umap_cases as uc
from tests.helpers import umap_np as un

MAX_RESTARTS = 200
SMALL_N = (4, 5, 9, 10, 17, 33)


# ------------------------------------------------------------------------------------------------ graphs, each with its dense spectrum
@functools.lru_cache(maxsize=None)
def graph(name):
    """(P, w, U, q0, S): the graph, ``eigh`` of its dense operator (descending) and the operator itself, computed once."""
    if name == "blobs":
        _, _, idx, dist = sn.connected_blobs()
        P = un.fuzzy_graph(idx, dist)[0]
    elif name == "hub":
        P = uc.layout_graph("hub")[0]
    elif name == "planted":
        P = sn.planted()
    elif name == "threshold":
        P = sn.threshold()
    else:
        kind, N, s = name.split("-")
        P = sn.ring(int(N), int(s)) if kind == "ring" else sn.complete(int(N))
    S, q0 = sn.dense_operator(P)
    w, U = np.linalg.eigh(S)
    return P, w[::-1].copy(), U[:, ::-1].copy(), q0, S


def start_block(N, ndim):
    return np.random.default_rng(ndim).standard_normal((N, ndim))


def _matrix():
    """(graph, ndim, m, tol), in the order of the table in DESIGN.md"""
    cases = [("blobs", b, 32, 1e-4) for b in range(1, 9)]
    cases += [("blobs", b, m, 1e-4) for b in (2, 3, 5, 8) for m in (2 * b + 2, 33, 64) if m >= 2 * b + 2]
    cases += [("hub", b, 32, 1e-4) for b in (1, 3, 4, 8)]
    cases += [("planted", b, 32, 1e-4) for b in (1, 3, 5, 8)]
    cases += [("threshold", b, 32, 1e-6) for b in (2, 3, 4, 5)]
    cases += [("ring-300-3", b, m, 1e-10) for b in (1, 2, 3, 4) for m in (32, 64)]
    return cases


def _small():
    return [(f"{kind}-{N}-1", b, 32, 1e-4) for kind in ("ring", "complete") for N in SMALL_N for b in range(1, min(N, 9))]


MATRIX = _matrix()
SMALL = _small()


def case_id(case):
    return "%s-ndim%d-m%d" % case[:3]


@functools.lru_cache(maxsize=None)
def port(name, ndim, m, tol, narrow_last_block=False):
    """The numpy statement of the method on the case's own start block, as the result dictionary of spectral_embedding."""
    P = graph(name)[0]
    return as_result(sb.solve(P, ndim, start_block(P.shape[0], ndim), tol, m, MAX_RESTARTS, narrow_last_block))


def as_result(solved):
    th, X, res, restarts, mults, converged = solved
    return {"vectors": X, "values": th, "laplacian_values": 1.0 - th, "residuals": res, "n_components": 1, "restarts": restarts,
            "multiplications": mults, "converged": converged}


# ------------------------------------------------------------------------------------------------ the properties every solve is held to
def check_solution(P, r, tol, w=None, q0=None, S=None):
    V, th = r["vectors"], r["values"]
    N, b = V.shape
    if q0 is None:
        w, _, q0 = sn.spectrum(P)
    assert r["n_components"] == 1 and r["converged"] and np.isfinite(V).all()
    assert np.allclose(r["laplacian_values"], 1.0 - th, rtol=0, atol=0)
    assert (np.diff(th) <= 1e-12).all()
    res = sn.residuals(P, V, th) if S is None else np.linalg.norm(S @ V - V * np.asarray(th)[None, :], axis=0)
    print(f"theta {th}, residuals host {res}, device {r['residuals']}, restarts {r['restarts']}, multiplications {r['multiplications']}")
    assert (res <= tol * np.abs(th) + 1e-12).all()
    assert np.allclose(r["residuals"], res, rtol=1e-3, atol=1e-13)                 # the reported ones are the true ones
    assert np.abs(V.T @ q0).max() <= 1e-10 and np.abs(V.T @ V - np.eye(b)).max() <= 1e-10
    assert np.array_equal(sn.canonical_sign(V), V)
    return res


def check_against_eigh(name, r, tol):
    """check_solution, every value against eigh's, and the vectors: the whole subspace by Davis-Kahan where a gap follows the
    last value asked for, vector by vector against its cluster of equal eigenvalues where ndim splits a degenerate one."""
    P, w, U, q0, S = graph(name)
    res = check_solution(P, r, tol, w, q0, S)
    V, th = r["vectors"], r["values"]
    N, b = V.shape
    assert np.abs(th - w[1:1 + b]).max() <= tol, (th, w[1:1 + b])
    if b + 1 >= N or w[b] - w[b + 1] > 1e-6:
        got, bound = sn.subspace_sine(V, U[:, 1:1 + b]), sn.subspace_bound(w, th, res)
        print(f"sine between the subspaces {got:.3e}, Davis-Kahan bound {bound:.3e}")
        assert got <= bound * (1 + 1e-6) + 1e-12
    else:
        for l in range(b):
            outside = np.abs(w - w[1 + l]) > 1e-9
            delta = float(np.abs(w[outside] - th[l]).min())
            got = sn.outside_cluster(V[:, l], th[l], w, U, delta)
            print(f"vector {l}: outside the {int((~outside).sum())} eigenvectors at its value {got:.3e}, bound {res[l] / delta:.3e}")
            assert got <= res[l] / delta * (1 + 1e-6) + 1e-12
    return res
