"""NMF on the device (include/gficf_nmf.h, libgficf_nmf.so): the solve bit for bit against the NumPy restatement
(tests/helpers/nmf_np.py), the half-step bit for bit from the device's own S and B, S and B within derived bounds, the chain
against its stages bit for bit, the loss, the planted matrix against the restatement, the pipeline, the rejections."""
import os
import sys
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gficf_amd  # noqa: E402
from gficf_amd import _nmf_lib  # noqa: E402
from tests.helpers import nmf_cases as nc  # noqa: E402
from tests.helpers import nmf_np as nn  # noqa: E402

pytestmark = pytest.mark.gpu
U = nc.U
CD_TOL = 1e-8
# The planted matrix, device against restatement: the largest relative difference of cells and w after iterations 1, 2, 5 and
# at the end, max |dev - ref| / max |ref|.  Measured on an MI355X: 2.95e-14, w after iteration 1 (see test_planted_matrix_against_the_restatement);
# accepted at ten times that, and never looser than 100 cd_tol = 1e-6.
PLANTED_MEASURED = 2.95e-14
PLANTED_TOL = min(10 * PLANTED_MEASURED, 100 * CD_TOL)


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ------------------------------------------------------------------ the solve
@pytest.mark.parametrize("k,M", nc.SOLVE_SHAPES)
def test_solve_bit_for_bit(k, M):
    S, B, H0 = nc.solve_case(k, M, warm=True)
    for h0 in (None, H0):
        got = gficf_amd.nnls(S, B, h0, ret_sweeps=True)
        want = nn.nnls_cd(S, B, h0)
        print(f"k = {k}, M = {M}, warm = {h0 is not None}: sweeps {want[1].min()} .. {want[1].max()}, zeros {float((want[0] == 0).mean()):.2f}, "
              f"max |dH| {np.abs(got[0] - want[0]).max():.3g}")
        assert same(got, want)


@pytest.mark.parametrize("k,M", [(2, 5), (64, 17), (65, 17), (128, 16)])
def test_solve_truncated_capped_and_degenerate(k, M):
    S, B, H0 = nc.solve_case(k, M, warm=True)
    for kw in (dict(cd_maxit=1), dict(cd_maxit=3), dict(cd_maxit=0), dict(cd_tol=0.0, cd_maxit=6)):
        for h0 in (None, H0):
            assert same(gficf_amd.nnls(S, B, h0, ret_sweeps=True, **kw), nn.nnls_cd(S, B, h0, **kw)), kw
    assert (gficf_amd.nnls(S, B, ret_sweeps=True, cd_tol=0.0, cd_maxit=6)[1] == 6).all()
    # B negative everywhere: nothing moves, exactly zero after one sweep
    H, sw = gficf_amd.nnls(S, -np.abs(B) - 1, ret_sweeps=True)
    assert (H == 0).all() and (sw == 1).all()
    # a zero diagonal entry: the coordinate stays 0, whatever the start, and nothing is NaN
    S0 = S.copy()
    S0[k // 2, k // 2] = 0.0
    for h0 in (None, H0 + 1):
        got = gficf_amd.nnls(S0, B, h0, ret_sweeps=True)
        assert same(got, nn.nnls_cd(S0, B, h0)) and (got[0][:, k // 2] == 0).all() and np.isfinite(got[0]).all()


@pytest.mark.parametrize("k,M,a", [(5, 37, 13), (65, 37, 16), (128, 40, 1)])
def test_solve_any_split_of_the_rows_and_twice(k, M, a):
    S, B, H0 = nc.solve_case(k, M, warm=True)
    whole = gficf_amd.nnls(S, B, H0, ret_sweeps=True)
    head, tail = gficf_amd.nnls(S, B[:a], H0[:a], ret_sweeps=True), gficf_amd.nnls(S, B[a:], H0[a:], ret_sweeps=True)
    assert np.array_equal(np.vstack([head[0], tail[0]]), whole[0]) and np.array_equal(np.concatenate([head[1], tail[1]]), whole[1])
    assert same(gficf_amd.nnls(S, B, H0, ret_sweeps=True), whole)


# ------------------------------------------------------------------ the half-step, S and B
CASES = {"300x200": (nc.sparse_300x200, 5), "40x1100": (nc.long_gene_40x1100, 5)}


@pytest.mark.parametrize("name", list(CASES))
def test_half_step_from_the_device_forms_and_their_bounds(name):
    """Both sides of an iteration: H from W on A, then W from H on A', warm-started.  The solve and the normalisation against
    half_step fed the device's own S and B: bit for bit.  S and B against W'W + ridge and A'W in numpy's f64 within
    n 2^-52 sum |a||x| per entry, n the number of terms (G + 1 for S with its ridge, the column's stored entries for B): both
    sums carry at most n 2^-53 sum |a||x| of rounding error each."""
    make, k = CASES[name]
    A = make()
    At = A.T.tocsc()
    At.sort_indices()
    G, N = A.shape
    W0 = np.random.default_rng(3).random((G, k))
    ridge = 1e-15
    dev = gficf_amd.nmf_half(A, W0)
    want = nn.half_step(dev["S"], dev["B"])
    assert np.array_equal(dev["y"], want["y"]) and np.array_equal(dev["d"], want["d"]) and np.array_equal(dev["sweeps"], want["sweeps"])
    assert dev["dead"] == 0 == want["dead"] and np.abs(dev["y"].sum(axis=0) - 1).max() < 1e-12
    dev2 = gficf_amd.nmf_half(At, dev["y"], Y=W0, d=dev["d"])
    want2 = nn.half_step(dev2["S"], dev2["B"], W0, dev["d"])
    assert np.array_equal(dev2["y"], want2["y"]) and np.array_equal(dev2["d"], want2["d"]) and np.array_equal(dev2["sweeps"], want2["sweeps"])
    if name == "40x1100":
        assert np.diff(At.indptr).max() > 1024                 # a gene of more than one segment
    for M_, X, r in ((A, W0, dev), (At, dev["y"], dev2)):
        n_in = M_.shape[0]
        Sref = X.T @ X + ridge * np.eye(k)
        sb = (n_in + 1) * U * (np.abs(X).T @ np.abs(X) + ridge * np.eye(k))
        Bref = np.asarray(M_.T @ X)
        nterm = np.diff(M_.indptr)[:, None]
        bb = nterm * U * np.asarray(abs(M_).T @ np.abs(X))
        rs, rb = np.abs(r["S"] - Sref) / sb, np.abs(r["B"] - Bref)[bb > 0] / bb[bb > 0]
        print(f"{name}, {n_in} rows in: S err / bound {rs.max():.3g}, B err / bound {rb.max() if rb.size else 0.0:.3g}")
        assert rs.max() <= 1 and (rb <= 1).all() and (r["B"][bb == 0] == 0).all()


def test_half_step_penalty_and_dead_factor():
    A = nc.sparse_300x200()
    W0 = np.random.default_rng(4).random((300, 5))
    plain, pen = gficf_amd.nmf_half(A, W0), gficf_amd.nmf_half(A, W0, l1=0.05)
    assert np.array_equal(pen["B"], plain["B"] - 0.05) and np.array_equal(pen["S"], plain["S"])
    assert np.array_equal(pen["y"], nn.half_step(pen["S"], pen["B"])["y"])
    W0[:, 2] = 0.0                                               # a zero column of the start: S[2][2] = ridge, B[:, 2] = 0, the factor is dead
    dead = gficf_amd.nmf_half(A, W0)
    assert dead["dead"] == 1 and dead["d"][2] == 0 and (dead["y"][:, 2] == 0).all() and np.isfinite(dead["y"]).all()
    assert np.array_equal(dead["y"], nn.half_step(dead["S"], dead["B"])["y"])


# ------------------------------------------------------------------ the chain
def run_quiet(*a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return gficf_amd.nmf(*a, **kw)


@pytest.mark.parametrize("name", list(CASES))
def test_chain_is_its_stages_in_order_and_repeats(name):
    make, k = CASES[name]
    A = make()
    At = A.T.tocsc()
    At.sort_indices()
    W0 = np.random.default_rng(5).random((A.shape[0], k))
    r = run_quiet(A, k, W0=W0, tol=0.0, maxit=3)
    W, H, d = W0, None, None
    for _ in range(3):
        s = gficf_amd.nmf_half(A, W, Y=H, d=d)
        H, d = s["y"], s["d"]
        s = gficf_amd.nmf_half(At, H, Y=W, d=d)
        W, d = s["y"], s["d"]
    assert r["iterations"] == 3 and not r["converged"]
    assert np.array_equal(r["w"], W) and np.array_equal(r["d"], d) and np.array_equal(r["h"], H.T) and np.array_equal(r["cells"], H * d)
    again = run_quiet(A, k, W0=W0, tol=0.0, maxit=3)
    assert all(np.array_equal(r[n], again[n]) for n in ("w", "d", "h", "delta"))
    assert np.array_equal(run_quiet(A, k, W0=W0, tol=0.0, maxit=2)["delta"], r["delta"][:2])


@pytest.mark.parametrize("name", list(CASES))
def test_loss_never_rises_and_is_its_entry(name):
    """Every coordinate step is an exact line minimisation and the rescaling leaves the product unchanged, so the loss can rise
    between two iterations only by the rounding of the two numbers compared.  The formula adds three non-negative sums; after
    the first iteration the fit is no worse than W = 0, so ||W d H|| <= 2 ||A||, the cross term is at most 2 ||A||^2 and the
    quadratic term at most 4 ||A||^2.  Their terms: nnz + 1 for ||A||^2; N k + (the longest column) + 2 for the cross term
    (counted twice: it enters as 2 x); k^2 + G + N + 3 for the quadratic term.  c is their sum weighted by those factors, and
    a difference of two losses carries twice that."""
    make, k = CASES[name]
    A = make()
    G, N = A.shape
    W0 = np.random.default_rng(6).random((G, k))
    r = run_quiet(A, k, W0=W0, tol=0.0, maxit=12, track_loss=True)
    nA = float((A.data ** 2).sum())
    c = (A.nnz + 1) + 2 * 2 * (N * k + int(np.diff(A.indptr).max()) + 2) + 4 * (k * k + G + N + 3)
    rise = np.diff(r["loss"]).max()
    print(f"{name}: relative loss {r['loss'][0] / nA:.4g} -> {r['loss'][-1] / nA:.4g}; largest rise {rise:.3g}, bound {2 * c * U * nA:.3g}")
    assert len(r["loss"]) == 12 and rise <= 2 * c * U * nA and r["loss"][-1] < r["loss"][0]
    terms = gficf_amd.nmf_loss(A, r["w"], r["d"], r["h"], ret_terms=True)
    assert terms[0] == r["loss"][-1] == gficf_amd.nmf_loss(A, r["w"], r["d"], r["h"])
    dense = nn.loss(A, r["w"], r["d"], r["h"])
    print(f"{name}: loss {terms[0]:.17g}, on the dense matrix {dense:.17g}, terms {terms[1:]}")
    assert abs(terms[0] - dense) <= 2 * c * U * nA and abs(terms[1] - nA) <= (A.nnz + 1) * U * nA


def test_planted_matrix_against_the_restatement():
    """A = W0 H0, 300 x 200, rank 4.  The restatement stops by tol after 6 iterations at a relative loss of 4.7e-5; the device
    must stop by tol too, after as many.  Beyond cd_tol the only sources of difference are the summation order of S and B
    and the sweep at which a row stops.  Measured on an MI355X: see PLANTED_MEASURED above."""
    A, W0 = nc.planted()
    ref = nn.nmf(A, 4, W0, keep=(1, 2, 5))
    dev = gficf_amd.nmf(A, 4, W0=W0, track_loss=True)
    assert ref["converged"] and dev["converged"] and dev["iterations"] == ref["iterations"] and dev["dead"] == 0
    worst = 0.0
    for it in (1, 2, 5, None):
        d_ = dev if it is None else run_quiet(A, 4, W0=W0, maxit=it)
        w_ref, c_ref = (ref["w"], ref["cells"]) if it is None else ref["history"][it]
        for what, got, want in (("w", d_["w"], w_ref), ("cells", d_["cells"], c_ref)):
            rel = np.abs(got - want).max() / np.abs(want).max()
            worst = max(worst, rel)
            print(f"planted, after {'the end' if it is None else it}: {what} relative difference {rel:.3g}")
    rel_loss = dev["loss"][-1] / float((A.data ** 2).sum())
    print(f"planted: largest relative difference {worst:.3g} (accepted {PLANTED_TOL:.3g}); {dev['iterations']} iterations, relative loss {rel_loss:.3g}")
    assert worst <= PLANTED_TOL and rel_loss < 1e-3 and np.abs(dev["delta"] - ref["delta"]).max() < 1e-9


# ------------------------------------------------------------------ the pipeline
@pytest.fixture(scope="module")
def trained():
    from gficf_amd import synth

    colptr, rowidx, x = synth.counts_csc(1500, 800)
    M = sp.csc_matrix((x, rowidx, colptr), shape=(1500, 800))
    data = gficf_amd.gficf(M[:, :750], normalize=False, verbose=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        data = gficf_amd.runNMF(data, dim=5, maxit=20)
    return M, data


def test_pipeline_on_the_nmf_cells():
    from gficf_amd import synth

    colptr, rowidx, x = synth.counts_csc(1500, 800)
    data = gficf_amd.gficf(sp.csc_matrix((x, rowidx, colptr), shape=(1500, 800)), normalize=False, verbose=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        data = gficf_amd.runNMF(data, dim=5, maxit=20, track_loss=True)
    p = data["pca"]
    G = data["gficf"].shape[0]
    assert p["type"] == "NMF" and p["cells"].shape == (800, 5) and p["genes"].shape == (G, 5) and p["h"].shape == (5, 800) and p["d"].shape == (5,)
    assert (p["cells"] >= 0).all() and np.isfinite(p["cells"]).all() and np.array_equal(p["cells"], (p["h"] * p["d"][:, None]).T)
    assert np.abs(p["genes"].sum(axis=0) - 1).max() < 1e-12 and p["centre"] is False and p["mean"] is None and data["dimPCA"] == 5
    assert (np.diff(p["nmf"]["loss"]) <= 0).all() and p["nmf"]["iterations"] == len(p["nmf"]["delta"]) <= 20
    data = gficf_amd.runReduction(data, n_epochs=50, verbose=False)
    emb = np.asarray(data["embedded"])
    assert emb.shape == (800, 2) and np.isfinite(emb).all()
    data = gficf_amd.clustcells(data, verbose=False)
    assert data["cluster"].shape == (800,) and data["community"].min() >= 1 and data["cluster.gene.rnk"].shape[0] == G


def test_new_cells_are_placed_by_the_projection(trained, monkeypatch):
    M, data = trained
    data = dict(data, pca=dict(data["pca"]))
    data = gficf_amd.runReduction(data, n_epochs=50, verbose=False)
    seen = []
    real = gficf_amd.api.nmf_project
    monkeypatch.setattr(gficf_amd.api, "nmf_project", lambda d, g, **kw: seen.append(g) or real(d, g, **kw))
    data = gficf_amd.embedNewCells(data, M[:, 750:], verbose=False)
    monkeypatch.undo()
    pred = data["pca"]["pred"]
    new = data["embedded"][data["embedded"]["predicted"] == "YES"]
    assert len(seen) == 1 and pred.shape == (50, 5) and (pred >= 0).all() and len(new) == 50 and np.isfinite(np.asarray(new[["X", "Y"]])).all()
    assert np.array_equal(pred, gficf_amd.nmf_project(data, seen[0])) and np.array_equal(pred, gficf_amd.nmf_project(data["pca"]["genes"], seen[0]))
    # a cell the training saw lands where a solve from zero puts it: close to its training row (which was warm-started)
    back = gficf_amd.nmf_project(data, data["gficf"][:, :20])
    assert np.abs(back - data["pca"]["cells"][:20]).max() <= 0.2 * data["pca"]["cells"].max()


def test_projection_is_the_solve_on_the_device_forms(trained):
    M, data = trained
    w, g = data["pca"]["genes"], data["gficf"][:, 100:133]
    k, G, n_new = 5, w.shape[0], 33
    s = gficf_amd.api._NmfState(g, k)
    ldk, lpk = _nmf_lib.ld(k), _nmf_lib.lp(k)
    H, S, B, sw = s.zeros(n_new, ldk), s.zeros(lpk, lpk), s.zeros(n_new, ldk), s.zeros(n_new, dtype=s.tc.int32)
    s.ops.nmf_project(G, n_new, s.colptr, s.rowidx, s.x, g.nnz, k, s.up(gficf_amd.api._nmf_pad(w, k, "w")), 1e-15, 1e-8, 100, H, s.ws, S=S, B=B, sweeps=sw)
    s.ops.nmf_sync(s.ws)
    want = nn.nnls_cd(S.cpu().numpy()[:k, :k], B.cpu().numpy()[:, :k])
    assert np.array_equal(H.cpu().numpy()[:, :k], want[0]) and np.array_equal(sw.cpu().numpy(), want[1]) and (H.cpu().numpy()[:, k:] == 0).all()
    host = gficf_amd.nmf_project(w, g, ret_sweeps=True)
    assert np.array_equal(host[0], want[0]) and np.array_equal(host[1], want[1])


# ------------------------------------------------------------------ the rejections
def test_rejections_by_status():
    A = nc.sparse_300x200()
    k = 5
    s = gficf_amd.api._NmfState(A, k)
    L, h = _nmf_lib.load(), s.ops._bind()
    tp = gficf_amd.api._tptr
    ldk = _nmf_lib.ld(k)
    W, Hh, d = s.up(gficf_amd.api._nmf_pad(np.random.default_rng(0).random((300, k)), k, "W")), s.zeros(200, ldk), s.zeros(k)
    delta, info = np.zeros(4), np.zeros(4, dtype=np.int64)
    dp, ip = delta.ctypes.data, info.ctypes.data
    nb = int(s.ws.numel())

    def chain(G=300, N=200, kk=k, tol=1e-4, maxit=2, l1w=0.0, l1h=0.0, ridge=1e-15, cd_tol=1e-8, cd_maxit=100, W0=W, ws=s.ws, ws_bytes=nb, cp=s.colptr):
        return L.gficf_nmf_device(h, G, N, tp(cp), tp(s.rowidx), tp(s.x), A.nnz, kk, tp(W0), tol, maxit, l1w, l1h, ridge, cd_tol, cd_maxit, 0, tp(W), tp(d),
                                  tp(Hh), dp, None, ip, tp(ws), ws_bytes)

    UNSUPPORTED, INVALID = 6, 1
    assert chain(kk=129) == UNSUPPORTED and chain(G=2 ** 31) == UNSUPPORTED and chain(N=2 ** 31) == UNSUPPORTED
    for kw in (dict(G=0), dict(N=0), dict(kk=0), dict(kk=128, N=100), dict(tol=-1.0), dict(maxit=-1), dict(l1w=-1.0), dict(l1h=-1.0), dict(ridge=-1.0),
               dict(cd_tol=-1.0), dict(cd_tol=float("nan")), dict(cd_maxit=-1), dict(W0=None), dict(cp=None), dict(ws=None), dict(ws_bytes=nb - 4096)):
        assert chain(**kw) == INVALID, kw
    S, B, sw = s.zeros(k, k), s.zeros(4, ldk), s.zeros(4, dtype=s.tc.int32)

    def solve(M=4, kk=k, lds=k, cd_tol=1e-8, cd_maxit=10, S_=S, ws_bytes=1024):
        return L.gficf_nnls_device(h, M, kk, tp(S_), lds, tp(B), None, cd_tol, cd_maxit, tp(B), tp(sw), tp(s.ws), ws_bytes)

    assert solve(kk=129) == UNSUPPORTED and solve(M=2 ** 31) == UNSUPPORTED
    for kw in (dict(M=0), dict(kk=0), dict(lds=k - 1), dict(cd_tol=-1.0), dict(cd_maxit=-1), dict(S_=None), dict(ws_bytes=512)):
        assert solve(**kw) == INVALID, kw
    assert L.gficf_nmf_loss_device(h, 300, 200, tp(s.colptr), tp(s.rowidx), tp(s.x), A.nnz, k, tp(W), tp(d), tp(Hh), None, tp(s.ws), nb) == INVALID
    assert L.gficf_nmf_project_device(h, 300, 200, tp(s.colptr), tp(s.rowidx), tp(s.x), A.nnz, 129, tp(W), 1e-15, 1e-8, 100, tp(Hh), None, None, None, tp(s.ws),
                                      nb) == UNSUPPORTED
    assert L.gficf_nmf_half_device(h, 300, 200, tp(s.colptr), tp(s.rowidx), tp(s.x), A.nnz, k, tp(W), tp(Hh), tp(d), 0, -1.0, 1e-15, 1e-8, 100, None, None, None,
                                   None, tp(s.ws), nb) == INVALID
    assert chain() == 0 and info[0] == 2                        # and the same call with nothing wrong goes through
    s.ops.nmf_sync(s.ws)


def test_deferred_errors_arrive_at_the_sync():
    A = nc.sparse_300x200()
    k, ldk = 5, _nmf_lib.ld(5)
    W0 = np.random.default_rng(0).random((300, k))

    def run(data=None, rowidx=None, W=W0):
        s = gficf_amd.api._NmfState(A, k)
        if data is not None:
            s.x = s.up(data)
        if rowidx is not None:
            s.rowidx = s.up(rowidx)
        Wd, H, d = s.up(gficf_amd.api._nmf_pad(W, k, "W")), s.zeros(200, ldk), s.zeros(k)
        r = s.ops.nmf(300, 200, s.colptr, s.rowidx, s.x, A.nnz, k, Wd, 1e-4, 5, 0.0, 0.0, 1e-15, 1e-8, 100, False, Wd, d, H, s.ws)
        assert r["iterations"] == 1                                # the first read-back saw the status word
        s.ops.nmf_sync(s.ws)

    neg = A.data.copy()
    neg[11] = -1.0
    with pytest.raises(gficf_amd.GficfError, match="negative entry") as e:
        run(data=neg)
    assert e.value.code == 8
    nan = A.data.copy()
    nan[11] = np.nan
    with pytest.raises(gficf_amd.GficfError, match="NaN or an infinite") as e:
        run(data=nan)
    assert e.value.code == 8
    bad = A.indices.copy()
    bad[5] = 300
    with pytest.raises(gficf_amd.GficfError, match="row index") as e:
        run(rowidx=bad)
    assert e.value.code == 3
    with pytest.raises(gficf_amd.GficfError, match="negative entry") as e:
        run(W=np.where(np.arange(1500).reshape(300, 5) == 7, -0.25, W0))
    assert e.value.code == 8
    # the sync cleared the word: the same workspace runs a good input afterwards (run() makes a new one each time; here one is reused)
    s = gficf_amd.api._NmfState(A, k)
    s.x = s.up(neg)
    Wd, H, d = s.up(gficf_amd.api._nmf_pad(W0, k, "W")), s.zeros(200, ldk), s.zeros(k)
    s.ops.nmf(300, 200, s.colptr, s.rowidx, s.x, A.nnz, k, Wd, 1e-4, 1, 0.0, 0.0, 1e-15, 1e-8, 100, False, Wd, d, H, s.ws)
    with pytest.raises(gficf_amd.GficfError):
        s.ops.nmf_sync(s.ws)
    s.ops.nmf_sync(s.ws)


def test_dead_factor_is_counted_and_stays_finite():
    A = nc.sparse_300x200()
    W0 = np.random.default_rng(8).random((300, 5))
    W0[:, 3] = 0.0
    r = run_quiet(A, 5, W0=W0, maxit=4, tol=0.0, track_loss=True)
    assert r["dead"] == 1 and r["d"][3] == 0 and (r["w"][:, 3] == 0).all() and (r["h"][3] == 0).all()
    assert all(np.isfinite(r[n]).all() for n in ("w", "d", "h", "cells", "delta", "loss"))


def test_reaching_maxit_warns_and_names_delta():
    A = nc.sparse_300x200()
    with pytest.warns(UserWarning, match=r"maxit = 2 iterations with delta = \d"):
        r = gficf_amd.nmf(A, 5, maxit=2)
    assert r["iterations"] == 2 and not r["converged"] and r["loss"] is None
