"""CPU: the numpy port of the exact truncated SVD (tests/helpers/svds_np.py) against LAPACK on the inputs of
tests/test_svds_gpu.py and on the case matrix of tests/helpers/svds_cases.py (every block width); the exported surface of libgficf_svds.so; argument errors of the Python mirror."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from tests.helpers import rsvd_np as rp
from tests.helpers import svds_cases as sc
from tests.helpers import svds_np as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 5


def _start(n, b, seed=SEED + 1):
    return np.random.default_rng(seed).standard_normal((n, b))


def _dev_d(M, r, k, centre=False):
    w = sn.dense_svd(M, k, centre)
    return float(np.abs(r["d"][:len(w["d"])] - w["d"]).max() / w["d"][0]), w


# name -> (matrix, k, m, centre, at least this many cycles)
PORT = {
    "restart_m40": (lambda: rp.planted_sparse(600, 320, 12, SEED), 10, 40, False, 2),
    "restart_m32": (lambda: rp.planted_sparse(600, 320, 12, SEED), 10, 32, False, 2),
    "transposed": (lambda: rp.planted_sparse(200, 640, 12, SEED), 10, 40, False, 2),
    "single_cycle": (lambda: rp.planted_sparse(300, 80, 6, SEED), 6, 80, False, 1),
    "k1": (lambda: rp.planted_sparse(300, 80, 6, SEED), 1, 24, False, 2),
    "full_83": (lambda: sp.csc_matrix(sp.random(83, 301, 0.2, random_state=np.random.default_rng(SEED))), 83, 83, False, 1),
    "flat": (lambda: sn.flat(SEED), 10, 40, False, 10),
    "centred": (lambda: rp.planted_sparse(600, 320, 12, SEED), 10, 40, True, 2),
    "segments": (lambda: sp.csc_matrix(sp.random(12, 3000, 0.9, random_state=np.random.default_rng(SEED))), 12, 12, False, 1),
}


@pytest.mark.parametrize("name", sorted(PORT))
def test_port_matches_lapack_to_rounding(name):
    make, k, m, centre, cycles = PORT[name]
    M = make()
    r = sn.svds(M, _start(min(M.shape), 8), k, m, centre=centre)
    dev, w = _dev_d(M, r, k, centre)
    # the values of a converged pair are stationary in the vectors: tol = 1e-10 on the residual leaves them at rounding level
    assert dev < 64 * rp.EPS, (name, dev)
    assert r["converged"] == k or r["exhausted"]
    assert r["cycles"] >= cycles and (r["cycles"] == 1) == (m == min(M.shape))
    g = r["genes"]
    assert np.abs(g.T @ g - np.eye(k)).max() < 1e-12
    i = np.argmax(np.abs(g), axis=0)
    assert (g[i, np.arange(k)] > 0).all() and (np.diff(r["d"]) <= 1e-12 * r["d"][0]).all()
    if centre:
        assert np.allclose(r["centre"], M.toarray().mean(axis=1), rtol=1e-13, atol=0)


@pytest.mark.parametrize("case", sc.ALL, ids=sc.case_id)
def test_port_matches_lapack_at_every_width_and_basis_size(case):
    """The rule of test_port_matches_lapack_to_rounding on the case matrix of tests/helpers/svds_cases.py: the port is the
    yardstick of tests/test_svds_widths_gpu.py at block widths other than 8, so it is held to LAPACK there first."""
    M, k = sc.matrix(case.matrix), case.k
    w, r = sc.lapack(case.matrix, k, case.centre), sc.port(case)
    dev = float(np.abs(r["d"][:len(w["d"])] - w["d"]).max() / w["d"][0])
    print(sc.case_id(case), "d", dev, "cycles", r["cycles"], "products", r["products"], "converged", r["converged"], "exhausted", r["exhausted"])
    assert dev < 64 * rp.EPS, (sc.case_id(case), dev)
    assert r["converged"] == k or r["exhausted"]
    nz = r["d"] > 0
    g = r["genes"][:, nz]
    assert np.abs(g.T @ g - np.eye(g.shape[1])).max() < 1e-12
    i = np.argmax(np.abs(r["genes"]), axis=0)
    assert (r["genes"][i, np.arange(k)][nz] > 0).all() and (np.diff(r["d"]) <= 1e-12 * r["d"][0]).all()
    if case.centre:
        assert np.allclose(r["centre"], M.toarray().mean(axis=1), rtol=1e-13, atol=0)
    if case.group == "NARROW":
        assert r["exhausted"] and r["cycles"] == 1 and (r["d"][sc.RANK:] == 0).all() and (r["d"][:min(k, sc.RANK)] > 0).all()
        assert (r["genes"][:, sc.RANK:] == 0).all() and (r["cells"][:, sc.RANK:] == 0).all()
    if case.group == "TINY":
        assert r["exhausted"] and r["cycles"] == 1 and case.m == min(M.shape)


def test_case_matrix_reaches_every_width_pitch_and_kept_count():
    """The lists are what the issue of the widths set: every b of the contract at the tightest basis and at the widest, more
    than 64 kept vectors, five chunks of rows, and only arguments the library accepts."""
    assert sorted({c.b for c in sc.WIDTHS if c.matrix == "planted" and not c.centre}) == list(range(1, 33))
    assert all(sn.check_args(min(sc.matrix(c.matrix).shape), c.k, c.b, c.m) for c in sc.ALL)
    assert len({sc.case_id(c) for c in sc.ALL}) == len(sc.ALL)
    assert all(min(c.k + c.b, c.m - c.b) > 64 for c in sc.MANY)                    # vectors kept at a restart from a full basis
    assert min(sc.matrix("tall").shape) == 1100 and -(-1100 // 256) == 5 and 220 % 16 and 220 % 8
    assert all(c.k == c.m == min(sc.matrix(c.matrix).shape) for c in sc.TINY)


def test_port_flat_spectrum_where_the_sketch_is_percent_level_off():
    M = sn.flat(SEED)
    w = sn.dense_svd(M, 11)
    assert w["d"][10] / w["d"][9] > 0.99                      # no gap behind the k-th value
    sk = rp.rsvd(M, np.random.default_rng(7).standard_normal((300, 20)), 10, q=2)
    assert np.abs(sk["d"] - w["d"][:10]).max() / w["d"][0] > 1e-3
    one = sn.svds(M, _start(300, 8), 10, 40, max_cycles=1)
    assert one["converged"] < 10 and one["cycles"] == 1 and one["residuals"].max() > 1e-3 and np.isfinite(one["cells"]).all()


def test_port_every_value_twice_and_rank_below_k():
    B = sp.random(21, 37, 0.4, random_state=np.random.default_rng(SEED), data_rvs=np.random.default_rng(SEED + 2).standard_normal)
    M = sp.csc_matrix(sp.block_diag([B, B]))
    r = sn.svds(M, _start(42, 8), 6, 24)
    dev, w = _dev_d(M, r, 6)
    assert dev < 64 * rp.EPS and r["converged"] == 6 and r["cycles"] > 5
    for g in ([0, 1], [2, 3], [4, 5]):
        assert rp.projector_diff(w["genes"][:, g], r["genes"][:, g]) < 1e-9
    M, d, U, V = rp.blocks(120, 60, [40, 30, 20], [10, 8, 6], [3.0, 2.0, 1.0])
    r = sn.svds(M, _start(60, 8), 5, 60)
    assert np.allclose(r["d"][:3], d, rtol=1e-13, atol=0) and (r["d"][3:] == 0).all() and r["exhausted"]
    assert (r["genes"][:, 3:] == 0).all() and (r["cells"][:, 3:] == 0).all()
    assert np.allclose(r["genes"][:, :3], V, rtol=0, atol=1e-13)


def test_port_schedule_and_argument_rule():
    assert sn.schedule(0, 320, 8, 40) == 5 and sn.schedule(18, 320, 8, 40) == 2 and sn.schedule(0, 83, 8, 83) == 11
    assert sn.check_args(320, 10, 8, 40) and sn.check_args(83, 83, 8, 83) and sn.check_args(12, 12, 8, 12)
    assert not sn.check_args(320, 10, 8, 25) and not sn.check_args(320, 10, 33, 128) and not sn.check_args(320, 10, 8, 129)
    assert not sn.check_args(320, 0, 8, 40) and not sn.check_args(4, 2, 8, 4)


# ------------------------------------------------------------------------------------------------ the library's surface
def _header_functions(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gficf_[a-z0-9_]+)\s*\(", src)))


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(re.findall(r" T (gficf_[a-z0-9_]+)$", out, re.M)))


def test_svds_library_exports_exactly_its_header():
    from gficf_amd import _svds_lib

    names = _header_functions("gficf_svds.h")
    assert names == ["gficf_svds_abi_version", "gficf_svds_device", "gficf_svds_host", "gficf_svds_sync", "gficf_svds_workspace_bytes"]
    assert sorted(_svds_lib.SIGNATURES) == names
    L = _svds_lib.load()
    assert L.gficf_svds_abi_version() == 1 == _svds_lib.ABI_VERSION
    if shutil.which("nm"):
        assert _exports(_svds_lib.LIB_PATH) == names
        needed = subprocess.run(["readelf", "-d", _svds_lib.LIB_PATH], capture_output=True, text=True).stdout if shutil.which("readelf") else ""
        assert "libgficf_pca" not in needed                  # the kernels are shared as text, not linked
    wb = L.gficf_svds_workspace_bytes
    # about 12 B per stored entry (the gene-major view) plus two bases of min(N, G) x m
    assert wb(2000, 5000, 1_000_000, 50, 8, 128) > 12 * 1_000_000 + 2 * 2000 * 128 * 8
    assert wb(-1, 5000, 1000, 10, 8, 40) == 0 and wb(2000, 5000, 1000, 0, 8, 40) == 0 and wb(2000, 5000, 1000, 10, 33, 128) == 0
    assert wb(2000, 5000, 1000, 10, 8, 129) == 0 and wb(2000, 5000, 1000, 10, 8, 25) == 0 and wb(2000, 5000, 1000, 10, 0, 40) == 0
    assert wb(20, 5000, 1000, 20, 8, 20) > 0 and wb(20, 5000, 1000, 10, 8, 21) == 0


def test_pca_and_core_libraries_are_unchanged():
    from gficf_amd import _lib, _pca_lib

    assert _pca_lib.load().gficf_pca_abi_version() == 1 and _lib.load().gficf_hip_abi_version() == 7
    if shutil.which("nm"):
        assert _exports(_pca_lib.LIB_PATH) == _header_functions("gficf_pca.h") and len(_exports(_pca_lib.LIB_PATH)) == 11
        assert len(_exports(_lib.LIB_PATH)) == 85


# ------------------------------------------------------------------------------------------------ the Python mirror
def test_argument_errors_of_the_mirror():
    import gficf_amd

    data = {"gficf": sp.csc_matrix(np.eye(4))}
    for fn in (gficf_amd.runPCA, gficf_amd.runLSA):
        with pytest.raises(ValueError, match='randomized must be True or "svds"'):
            fn(dict(data), dim=2, randomized="exact")
        with pytest.raises(NotImplementedError, match="randomized=True") as e:
            fn(dict(data), dim=2, randomized=False)
        assert '"svds"' in str(e.value)
    with pytest.raises(ValueError, match='randomized must be True or "svds"'):
        gficf_amd.computePCADim(dict(data), randomized="rsvd")
    with pytest.raises(NotImplementedError, match="randomized=True") as e:
        gficf_amd.computePCADim(dict(data), randomized=False)
    assert '"svds"' in str(e.value)
    with pytest.raises(ValueError, match="start must have"):
        gficf_amd.svds(data["gficf"], 2, start=np.zeros((3, 2)))
    with pytest.raises(ValueError, match="start must have"):
        gficf_amd.svds(data["gficf"], 2, start=np.zeros(4))
    assert "svds" in gficf_amd.__all__ if hasattr(gficf_amd, "__all__") else hasattr(gficf_amd, "svds")


@pytest.mark.skipif(__import__("gficf_amd").device_count() != 0, reason="GPU present")
def test_entries_fail_with_no_device_without_a_gpu():
    import gficf_amd

    M = sp.csc_matrix(np.eye(6))
    for call in (lambda: gficf_amd.svds(M, 2), lambda: gficf_amd.runPCA({"gficf": M}, dim=2, randomized="svds")):
        with pytest.raises(gficf_amd.GficfError) as e:
            call()
        assert e.value.status == "GFICF_ERR_NO_DEVICE"
