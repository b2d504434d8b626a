"""CPU: the marker-gene oracle (tests/helpers/markers_np.py) against itself, scipy and hand-derived values; R's p.adjust;
the exported surface of libgficf_markers.so."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.helpers import markers_np as mk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _labels(rng, N, C):
    ids = np.concatenate([np.arange(C), rng.integers(0, C, N - C)])
    rng.shuffle(ids)
    return ids


@pytest.mark.parametrize("kind", ["counts", "cpm", "signed"])
def test_literal_and_shared_sort_forms_agree(kind):
    rng = np.random.default_rng({"counts": 1, "cpm": 2, "signed": 3}[kind])
    G, N, C = 12, 61, 4
    M = rng.poisson(0.8, (G, N)).astype(np.float64)
    if kind == "cpm":
        M = M / np.maximum(M.sum(0), 1) * 1e6
    if kind == "signed":
        M[rng.random((G, N)) < 0.2] *= -1
        M[0, :5] = -0.0
    M[1] = 3.0                                           # one distinct value
    ids = _labels(rng, N, C)
    a = mk.markers_literal(M, ids, C)
    b = mk.markers_shared(M, ids, C)
    for k in ("U1", "U2", "T", "p"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(np.isnan(a["z"]), np.isnan(b["z"]))
    assert np.array_equal(a["z"][~np.isnan(a["z"])], b["z"][~np.isnan(b["z"])])
    assert np.allclose(a["lfc"], b["lfc"], rtol=0, atol=1e-12)
    assert (a["p"][1] == 1.0).all()


@pytest.mark.parametrize("kind", ["counts", "cpm", "signed", "explicit_zeros", "one_value"])
def test_sparse_oracle_equals_the_shared_sort_and_literal_forms(kind):
    import scipy.sparse as sp

    rng = np.random.default_rng({"counts": 21, "cpm": 22, "signed": 23, "explicit_zeros": 24, "one_value": 25}[kind])
    G, N, C = 14, 73, 5
    D = rng.poisson(0.8, (G, N)).astype(np.float64)
    if kind == "cpm":
        D = D / np.maximum(D.sum(0), 1) * 1e6
    if kind == "signed":
        D[rng.random((G, N)) < 0.25] *= -1.5
        D[0, :6] = -0.0
    D[1] = 3.0                                           # one distinct value, no zero
    D[2] = 0.0                                           # all zero
    D[3, :N - 2] = 0.0                                   # nearly all zero
    if kind == "one_value":
        D[D != 0] = 2.5
    S = sp.csc_matrix(D)
    if kind in ("explicit_zeros", "signed"):             # stored zeros (and -0.0) next to the non-zeros
        coo = S.tocoo()
        zr, zc = np.nonzero(D == 0)
        pick = rng.random(len(zr)) < 0.3
        zv = np.where(np.arange(pick.sum()) % 2 == 0, 0.0, -0.0)
        S = sp.csc_matrix((np.concatenate([coo.data, zv]), (np.concatenate([coo.row, zr[pick]]), np.concatenate([coo.col, zc[pick]]))),
                          shape=(G, N))
        assert S.nnz > np.count_nonzero(D)
    ids = _labels(rng, N, C)
    a = mk.markers_literal(D, ids, C)
    b = mk.markers_shared(S, ids, C)
    c = mk.markers_sparse(S, ids, C)
    for ref in (a, b):
        for k in ("U1", "U2", "T", "p"):
            assert np.array_equal(ref[k], c[k]), k
        assert np.array_equal(np.isnan(ref["z"]), np.isnan(c["z"]))
        assert np.array_equal(ref["z"][~np.isnan(ref["z"])], c["z"][~np.isnan(c["z"])])
        assert np.allclose(ref["lfc"], c["lfc"], rtol=0, atol=1e-12)
    assert (c["p"][1] == 1.0).all() and (c["p"][2] == 1.0).all()


def test_sparse_oracle_at_scale_and_on_wide_ranges():
    """A million genes in seconds; the rest's sum never cancels (a cluster holding a huge value); T near 2^63."""
    import scipy.sparse as sp

    rng = np.random.default_rng(26)
    G, N = 1_000_000, 40
    nnz = 2_000_000
    S = sp.csc_matrix((rng.integers(1, 5, nnz).astype(np.float64), (rng.integers(0, G, nnz), rng.integers(0, N, nnz))), shape=(G, N))
    S.sum_duplicates()
    ids = _labels(rng, N, 3)
    r = mk.markers_sparse(S, ids, 3)
    for g in (0, 17, G - 1):
        w = mk.markers_shared(S[g], ids, 3)
        for k in ("U1", "U2", "T", "p"):
            assert np.array_equal(w[k][0], r[k][g]), k
    N = 1000
    row = rng.random(N) * 3
    row[7] = 1e40
    ids = _labels(rng, N, 4)
    r = mk.markers_sparse(sp.csc_matrix(row[None, :]), ids, 4)
    for c in range(4):
        s1, s2 = math.fsum(row[ids == c]), math.fsum(row[ids != c])
        n1 = int((ids == c).sum())
        assert r["lfc"][0, c] == pytest.approx(math.log2(((s1 + n1) / n1) / ((s2 + N - n1) / (N - n1))), abs=1e-12)
    N = 2_097_151
    row = np.full(N, 2.0)
    row[:3] = [0.0, 1.0, 5.0]
    ids = np.zeros(N, dtype=np.int64)
    ids[5] = 1
    r = mk.markers_sparse(sp.csc_matrix(row[None, :]), ids, 2)
    t = N - 3
    assert r["T"][0, 0] == (t ** 3 - t) and r["T"][0, 0] > 2 ** 62


def test_oracle_matches_scipy_where_the_quirks_do_not_apply():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(5)
    checked = 0
    for _ in range(200):
        n1, n2 = int(rng.integers(2, 30)), int(rng.integers(2, 30))
        if (n1 * n2) % 2:
            continue
        x = rng.poisson(1.5, n1).astype(float)
        y = rng.poisson(2.0, n2).astype(float)
        r = mk.wmu_literal(x, y)
        if r["U1"] == r["U2"] or len(np.unique(np.concatenate([x, y]))) < 2:
            continue
        want = stats.mannwhitneyu(x, y, use_continuity=True, alternative="two-sided", method="asymptotic").pvalue
        assert r["p"] == pytest.approx(want, rel=1e-9, abs=1e-300)
        checked += 1
    assert checked > 50


def test_quirk_equal_u_gives_p_below_one():
    r = mk.wmu_literal([1, 4], [2, 3])
    assert r["U1"] == r["U2"] == 2.0
    assert r["p"] == math.erfc(0.5 / math.sqrt(5 / 3) / math.sqrt(2))
    assert r["p"] < 1


def test_quirk_odd_n1_n2_floors_mu():
    # n1 = 1, n2 = 3: mu = floor(3 / 2) = 1, not 1.5.  x = [10] ranks 4: U1 = 3, U2 = 0 -> z = (0 - 1 + 0.5) / sigma
    r = mk.wmu_literal([10], [1, 2, 3])
    assert (r["U1"], r["U2"]) == (3.0, 0.0)
    sig = math.sqrt((3 / 12) * (5 - 0 / 12))
    assert r["z"] == -0.5 / sig
    assert r["p"] == math.erfc(0.5 / sig / math.sqrt(2))


def test_single_distinct_value_and_complete_separation():
    assert mk.wmu_literal([0, 0, 0], [0, 0])["p"] == 1.0
    assert mk.wmu_literal([-0.0, 0.0], [0.0])["p"] == 1.0
    # complete separation, no ties: U1 = n1 n2, U2 = 0, z = (0 - mu + 0.5) / sqrt(n1 n2 (n1 + n2 + 1) / 12)
    n1, n2 = 5, 7
    r = mk.wmu_literal(np.arange(10, 15), np.arange(7))
    assert (r["U1"], r["U2"], r["T"]) == (35.0, 0.0, 0)
    z = (0 - 17 + 0.5) / math.sqrt((n1 * n2 / 12) * (n1 + n2 + 1))
    assert r["z"] == z


def test_negative_values_rank_below_the_zero_group():
    r = mk.wmu_literal([-1.0, 0.0], [0.0, 2.0])
    # sorted: -1 (rank 1), 0 0 (rank 2.5 each), 2 (rank 4): R1 = 3.5, R2 = 6.5
    assert (r["U1"], r["U2"], r["T"]) == (0.5, 3.5, 6)


def test_p_adjust_hand_values():
    from gficf_amd.api import p_adjust_fdr

    p = np.array([0.01, 0.04, 0.03, 0.2])
    # ascending 0.01, 0.03, 0.04, 0.2: n p / i = 0.04, 0.06, 0.05333.., 0.2 -> cummin from the top: 0.04, 0.05333.., 0.05333.., 0.2
    want = np.array([0.04, 4 / 3 * 0.04, 4 / 3 * 0.04, 0.2])
    for f in (p_adjust_fdr, mk.p_adjust_bh):
        assert np.allclose(f(p), want, rtol=1e-15, atol=0)
    ties = np.array([0.5, 0.01, 0.5, 0.9])
    assert np.allclose(p_adjust_fdr(ties), [2 / 3, 0.04, 2 / 3, 0.9], rtol=1e-15, atol=0)
    assert p_adjust_fdr(np.array([0.9, 0.95]))[1] == 0.95 and p_adjust_fdr(np.array([1.0, 1.0]))[0] == 1.0
    rng = np.random.default_rng(3)
    q = rng.random(300) ** 3
    assert np.array_equal(p_adjust_fdr(q), mk.p_adjust_bh(q))


def _header_functions():
    src = open(os.path.join(ROOT, "include", "gficf_markers.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gficf_[a-z0-9_]+)\s*\(", src)))


def test_markers_library_exports_exactly_its_header():
    from gficf_amd import _markers_lib

    names = _header_functions()
    assert len(names) == 6
    assert sorted(_markers_lib.SIGNATURES) == names
    L = _markers_lib.load()
    assert L.gficf_markers_abi_version() == 1
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", _markers_lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert sorted(set(re.findall(r" T (gficf_[a-z0-9_]+)$", out, re.M))) == names
    assert L.gficf_cluster_markers_workspace_bytes(100, 1000, 5000, 5) > 5000 * 50
    assert L.gficf_cluster_markers_workspace_bytes(-1, 1000, 5000, 5) == 0


def test_find_cluster_markers_argument_errors():
    import gficf_amd

    with pytest.raises(ValueError, match="Please identify cluster first"):
        gficf_amd.findClusterMarkers({"rawCounts": np.eye(2)})
    with pytest.raises(ValueError, match="No raw/normalized counts stored"):
        gficf_amd.findClusterMarkers({"community": np.array([1, 2])})
    with pytest.raises(NotImplementedError, match="hvg=False"):
        gficf_amd.findClusterMarkers({"community": np.array([1, 2]), "rawCounts": np.eye(2)}, hvg=True)
