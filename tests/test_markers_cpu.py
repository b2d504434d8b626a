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
