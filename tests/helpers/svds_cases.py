"""What tests/test_svds_gpu.py, tests/test_svds_widths_gpu.py and tests/test_svds_cpu.py share: the figures and properties every
truncated SVD is held to, the device form of the call, and the matrix of (matrix, k, b, m, centre) at which the solve is run at
every block width b and at the basis sizes m where its kernels change path ("svds at every width").  The same cases
are put to the device and to the numpy port of the method (tests/helpers/svds_np.py): the port proves that a case is solvable by
the method and sets the cycles and products allowed.  LAPACK and the port are computed once per case and never written to."""
import functools
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

from tests.helpers import rsvd_np as rp
from tests.helpers import svds_np as sn

EPS = rp.EPS
TOL = 1e-10
SEED = 5
RANK = 20                                                      # of the matrix "rank20"


def _start(n, b, seed=SEED + 1):
    return np.random.default_rng(seed).standard_normal((n, b))


def _groups(d, gap):
    """Runs of consecutive components whose values are closer than gap."""
    out, cur = [], [0]
    for i in range(1, len(d)):
        if d[i - 1] - d[i] < gap:
            cur.append(i)
        else:
            out.append(cur)
            cur = [i]
    out.append(cur)
    return out


def _figures(want, r):
    """d relative to d[0]; cells / d[0] and genes, sign-aligned, a group of (nearly) coinciding values by its projector."""
    d0 = want["d"][0]
    kk = int((want["d"] > 1e-9 * d0).sum())                  # (the zero components of a rank below k: asserted apart)
    fd = float(np.abs(r["d"][:len(want["d"])] - want["d"]).max() / d0)
    fc = fg = 0.0
    for g in _groups(want["d"][:kk], 1e-6 * d0):
        wg, wc = want["genes"][:, g], want["cells"][:, g]
        rg, rc = r["genes"][:, g], r["cells"][:, g]
        if len(g) == 1:
            fg = max(fg, float(np.abs(wg - rp.align(wg, rg)).max()))
            fc = max(fc, float(np.abs(wc - rp.align(wc, rc)).max() / d0))
        else:
            dg = want["d"][g]
            fg = max(fg, rp.projector_diff(wg, rg))
            fc = max(fc, rp.projector_diff(wc / dg, rc / r["d"][g]) * float(dg[0] / d0))
    return {"d": fd, "cells": fc, "genes": fg}


def _At(M, centre):
    A = sp.csc_matrix(M).T.toarray()
    return A - A.mean(axis=0) if centre else A


def _properties(M, centre, r):
    """genes'genes = I over the non-zero components, cells = At genes relative to d[0], on the host in f64."""
    nz = r["d"] > 0
    g, d0 = r["genes"][:, nz], r["d"][0]
    return {"orth": float(np.abs(g.T @ g - np.eye(g.shape[1])).max()),
            "cells": float(np.abs(r["cells"] - _At(M, centre) @ r["genes"]).max() / d0)}


def _device_form(M, k, b, m, centre, start, max_cycles=1000, ws_cut=0, colptr=None, x=None):
    import torch

    from gficf_amd.api import HipOps

    G, N = M.shape
    ops = HipOps(0)
    dev = torch.device("cuda", 0)
    cp, ri, xv = (torch.from_numpy(a).to(dev) for a in ((M.indptr if colptr is None else colptr).astype(np.int64), M.indices.astype(np.int32),
                                                        M.data if x is None else x))
    sd = torch.from_numpy(np.ascontiguousarray(start.T)).to(dev)
    d = torch.zeros(k, dtype=torch.float64, device=dev)
    cells = torch.zeros((k, N), dtype=torch.float64, device=dev)
    genes = torch.zeros((k, G), dtype=torch.float64, device=dev)
    resid = torch.zeros(k, dtype=torch.float64, device=dev)
    info = torch.zeros(4, dtype=torch.int64, device=dev)
    mean = torch.zeros(G, dtype=torch.float64, device=dev)
    need = ops.svds_workspace_bytes(G, N, M.nnz, k, b, m)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    ops.svds(G, N, cp, ri, xv, centre, sd, k, b, m, TOL, max_cycles, ws[: need - ws_cut], d, cells, genes, resid, info, mean)
    ops.svds_sync(ws)
    return {"d": d.cpu().numpy(), "cells": cells.cpu().numpy().T, "genes": genes.cpu().numpy().T, "residuals": resid.cpu().numpy(),
            "info": info.cpu().numpy(), "centre": mean.cpu().numpy()}


# ------------------------------------------------------------------------------------------------ the checks two files share
def check_properties(name, M, centre, k, port, got):
    """The body of test_properties_orthonormal_genes_cells_sign_rule_order."""
    pp, pg = _properties(M, centre, port), _properties(M, centre, got)
    print(name, "port", pp, "device", pg)
    for q in pp:
        assert pg[q] <= rp.tolerance(pp[q]), (name, q, pg[q], pp[q])
    nz = got["d"] > 0
    i = np.argmax(np.abs(got["genes"]), axis=0)
    assert (got["genes"][i, np.arange(k)][nz] > 0).all()
    assert (got["d"][:-1] >= got["d"][1:] * (1 - 1e-12)).all()
    assert (got["genes"][:, ~nz] == 0).all() and (got["cells"][:, ~nz] == 0).all()
    with np.errstate(divide="ignore", invalid="ignore"):
        assert np.array_equal(got["u"], np.where(got["d"] > 0, got["cells"] / got["d"], 0.0))


def check_direct_residual(name, M, centre, port, got):
    """The body of test_direct_residual_on_the_host."""
    tau = rp.tau(max(M.shape))
    rg, rq = sn.direct_residual(M, got, centre), sn.direct_residual(M, port, centre)
    bound = np.maximum(TOL * got["d"] ** 2, tau * got["d"][0] ** 2) + rq
    print(name, "device", rg.max() / got["d"][0] ** 2, "port", rq.max() / got["d"][0] ** 2, "worst ratio", (rg / bound).max())
    assert (rg <= bound).all(), (name, rg, bound)


# ------------------------------------------------------------------------------------------------ matrices (genes x cells CSC)
@functools.lru_cache(maxsize=None)
def matrix(name):
    if name == "planted":
        return rp.planted_sparse(600, 320, 12, SEED)
    if name == "transposed":
        return rp.planted_sparse(200, 640, 12, SEED)
    if name == "flat":
        return sn.flat(SEED)
    if name == "tall":
        return rp.planted_sparse(2000, 1100, 12, SEED)
    if name == "rank20":
        A = np.random.default_rng(3).standard_normal((150, RANK)) @ np.random.default_rng(4).standard_normal((RANK, 90))
        return sp.csc_matrix(A.T)
    kind, G, N = name.split("-")                              # dense-G-N
    assert kind == "dense"
    return sp.csc_matrix(np.random.default_rng(SEED).standard_normal((int(G), int(N))))


Case = namedtuple("Case", "group matrix k b m centre")


def _widths():
    out = [Case("WIDTHS", "planted", 10, b, m, False) for b in range(1, 33) for m in (10 + 2 * b, 128)]
    out += [Case("WIDTHS", "planted", 10, b, m, True) for b in (5, 17, 32) for m in (10 + 2 * b, 128)]
    out += [Case("WIDTHS", "transposed", 10, b, m, False) for b in (1, 3, 7, 9, 16, 17, 31, 32) for m in (10 + 2 * b, 128)]
    return out


def _hard():
    out = [Case("HARD", "flat", 10, b, 128, False) for b in (3, 7, 9, 16, 17, 25, 32)]
    return out + [Case("HARD", "flat", 10, b, 10 + 2 * b, False) for b in (9, 16, 17, 25, 32)]


def _tiny():
    out = []
    for G, N in ((1, 5), (5, 1), (2, 7), (3, 3)):
        n = min(G, N)
        out += [Case("TINY", f"dense-{G}-{N}", n, b, n, False) for b in range(1, n + 1)]
    out += [Case("TINY", "dense-32-50", 32, 32, 32, False), Case("TINY", "dense-50-32", 32, 32, 32, False)]
    return out + [Case("TINY", "dense-33-50", 33, 32, 33, False)]


WIDTHS = _widths()
HARD = _hard()
MANY = [Case("MANY", mat, k, b, 128, False) for mat in ("flat", "planted") for k, b in ((70, 8), (70, 16), (96, 16), (64, 32), (65, 31))]
TALL = [Case("TALL", "tall", 10, b, m, False) for b, m in ((5, 40), (12, 40), (32, 128))]
# k = 5 below the rank; the last asks for more than the rank has, so that the zeros beyond it are there to be looked at
NARROW = [Case("NARROW", "rank20", 5, b, m, False) for b, m in ((7, 90), (12, 90), (12, 48), (32, 90))] + [Case("NARROW", "rank20", 24, 12, 90, False)]
TINY = _tiny()
ALL = WIDTHS + HARD + MANY + TALL + NARROW + TINY
ONE_CYCLE_B = (1, 2, 5, 7, 9, 12, 16, 17, 24, 31, 32)


def case_id(c):
    return "%s-%s-k%d-b%d-m%d" % c[:5] + ("-centred" if c.centre else "")


def _freeze(r):
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def lapack(name, k, centre):
    return _freeze(sn.dense_svd(matrix(name), k, centre))


def start_of(c):
    return _start(min(matrix(c.matrix).shape), c.b)


@functools.lru_cache(maxsize=None)
def port(c, max_cycles=1000):
    return _freeze(sn.svds(matrix(c.matrix), start_of(c), c.k, c.m, tol=TOL, max_cycles=max_cycles, centre=c.centre))


def steps_of_one_cycle(c):
    return sn.schedule(0, min(matrix(c.matrix).shape), c.b, c.m)


# ------------------------------------------------------------------------------------------------ the vectors' bound
def vector_bound(c):
    """2 max_i max(tol d_i^2, tau d_1^2) / gap_i over the non-zero components asked for: Davis-Kahan for a pair stopped by the
    criterion of include/gficf_svds.h (residual of C = A'A at most max(tol theta_i, tau theta_1)).  gap_i: from d_i^2 to the
    nearest d_j^2 outside i's group of (nearly) coinciding values, the groups being those of _figures.  From LAPACK's spectrum
    and the arguments alone."""
    M = matrix(c.matrix)
    w = lapack(c.matrix, c.k, c.centre)
    d, d2 = w["d"], w["d_all"] ** 2
    kk = int((d > 1e-9 * d[0]).sum())
    tau = rp.tau(max(M.shape))
    worst = 0.0
    for g in _groups(d[:kk], 1e-6 * d[0]):
        others = np.delete(d2, g)
        for i in g:
            gap = float(np.abs(others - d2[i]).min()) if len(others) else np.inf
            worst = max(worst, 2.0 * float(max(TOL * d2[i], tau * d2[0])) / gap if gap > 0 else np.inf)
    return worst
