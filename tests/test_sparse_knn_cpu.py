"""No GPU: the NumPy oracle of the sparse search (tests/helpers/sparse_knn_oracle.py) against a brute-force loop, the closed form
of the ring against the oracle, the header against the loader, the shape rule, and everything the Python mirror decides before
the first call into the library (find_nn_sparse's argument checks, the refusals that name runReductionSparse, its keywords)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import gficf_amd
from gficf_amd import GficfError, _sparse_knn_lib
from tests.helpers import sparse_knn_oracle as so
from tests.helpers import sparse_knn_ring as ring

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("metric", so.METRICS)
def test_oracle_against_a_brute_force_loop(metric):
    M = so.case(30, 40, 0.3, 1)
    want = so.oracle(M, metric, 8)
    idx, dist = so.brute_force(M, metric, 8)
    assert so.compare({"idx": idx, "dist": dist}, want, metric) == []
    assert np.array_equal(idx, want["idx"])


def test_comparison_rule_catches_a_lost_neighbour_and_a_wrong_distance():
    M = so.case(30, 40, 0.3, 2)
    want = so.oracle(M, "euclidean", 8)
    far = so.table(want["q"], "euclidean", 9)
    lost = {"idx": np.delete(far[0], 3, axis=1), "dist": np.delete(far[1], 3, axis=1)}         # every row skips its 4th neighbour
    with pytest.raises(AssertionError, match="differ from the oracle"):
        so.compare(lost, want, "euclidean")
    off = {"idx": want["idx"].copy(), "dist": want["dist"].copy()}
    off["dist"][5, 7] *= 1 + 2.0 ** -20
    with pytest.raises(AssertionError, match="tolerance"):
        so.compare(off, want, "euclidean")


@pytest.mark.parametrize("metric", ("euclidean", "cosine"))
def test_ring_closed_form_is_the_oracles(metric):
    M = ring.ring_matrix(200, 8)
    idx, dist = ring.ring_expected(200, 8, 3, metric)
    want = so.oracle(M, metric, 7)
    assert so.compare({"idx": idx, "dist": dist}, want, metric) == [] and np.array_equal(idx, want["idx"])


# ------------------------------------------------------------------------------------------------ the library's surface
def test_header_and_loader_name_the_same_entries():
    text = open(os.path.join(ROOT, "include", "gficf_sparse_knn.h")).read()
    body = re.sub(r"/\*.*?\*/", "", text[text.index("extern \"C\""):], flags=re.S)
    declared = {m.group(1): m.group(2) for m in re.finditer(r"\b(gficf_sparse_knn_\w+)\s*\(([^)]*)\)\s*;", body)}
    assert set(declared) == set(_sparse_knn_lib.SIGNATURES) and len(declared) == 6
    for name, args in declared.items():
        n = 0 if args.strip() == "void" else args.count(",") + 1
        assert n == len(_sparse_knn_lib.SIGNATURES[name][1]), name
    assert "#define GFICF_SPARSE_KNN_ABI_VERSION 1" in text and _sparse_knn_lib.ABI_VERSION == 1
    assert re.search(r"#define\s+GFICF_SPARSE_KNN_LANES\s+%d\b" % _sparse_knn_lib.LANES, text)
    assert re.search(r"#define\s+GFICF_SPARSE_KNN_LDS_FLOATS\s+%d\b" % _sparse_knn_lib.LDS_FLOATS, text)
    core = open(os.path.join(ROOT, "include", "gficf_hip.h")).read()
    assert re.search(r"#define\s+GFICF_HIP_ABI_VERSION\s+7\b", core)
    L = _sparse_knn_lib.load()
    assert L.gficf_sparse_knn_abi_version() == 1
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", _sparse_knn_lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert sorted(set(re.findall(r" T (gficf_[a-z0-9_]+)$", out, re.M))) == sorted(_sparse_knn_lib.SIGNATURES)
    wb = L.gficf_sparse_knn_workspace_bytes
    # the f32 copy of the values, two scalars per cell, one list of k keys per query and slice
    assert wb(5000, 54000, 1_000_000, 16, 54000) >= 4 * 1_000_000 + 16 * 54000 + 8 * 16 * 54000
    assert wb(5000, 54000, 1_000_000, 16, 0) > 0 and wb(5000, 54000, 1_000_000, 16, 54001) == 0
    assert wb(0, 10, 5, 2, 10) == 0 and wb(_sparse_knn_lib.LDS_FLOATS + 1, 10, 5, 2, 10) == 0 and wb(10, 10, 5, 129, 10) == 0


def test_shape_rule():
    top = gficf_amd.find_nn_sparse_shape(1, 300, 16)
    assert top == {"tile_queries": 8, "slices": 1, "max_genes": _sparse_knn_lib.LDS_FLOATS}
    last = 8
    for G in list(range(1, 40000, 509)) + [top["max_genes"]]:
        if G > top["max_genes"]:
            with pytest.raises(GficfError) as e:
                gficf_amd.find_nn_sparse_shape(G, 300, 16)
            assert e.value.status == "GFICF_ERR_UNSUPPORTED" and str(top["max_genes"]) in str(e.value)
            continue
        s = gficf_amd.find_nn_sparse_shape(G, 300, 16)
        assert s["tile_queries"] in (1, 2, 4, 8) and s["tile_queries"] <= last and s["max_genes"] == top["max_genes"]
        assert G * s["tile_queries"] <= _sparse_knn_lib.LDS_FLOATS < G * s["tile_queries"] * 2 or s["tile_queries"] == 8
        last = s["tile_queries"]
    assert last == 1
    for N in (1, 2, 255, 300, 1000, 2047, 2048, 54000):
        s = gficf_amd.find_nn_sparse_shape(300, N, 1)
        assert s == gficf_amd.find_nn_sparse_shape(300, N, 1) and 1 <= s["slices"] <= max(1, N // 256)   # no slice under 256 candidates
    assert gficf_amd.find_nn_sparse_shape(300, 1000, 16)["slices"] > 1 and gficf_amd.find_nn_sparse_shape(300, 54000, 16)["slices"] == 1
    for bad, status in (((300, 0, 1), "GFICF_ERR_INVALID_ARG"), ((300, 10, 11), "GFICF_ERR_INVALID_ARG"), ((300, 600, 129), "GFICF_ERR_UNSUPPORTED")):
        with pytest.raises(GficfError) as e:
            gficf_amd.find_nn_sparse_shape(*bad)
        assert e.value.status == status


# ------------------------------------------------------------------------------------------------ the mirror's checks
def test_find_nn_sparse_argument_checks():
    M = so.case(30, 40, 0.3, 1)
    with pytest.raises(ValueError, match="metric must be one of"):
        gficf_amd.find_nn_sparse(M, 5, metric="chebyshev")
    with pytest.raises(ValueError, match="k must be at least 1"):
        gficf_amd.find_nn_sparse(M, 0)
    with pytest.raises(ValueError, match="2-d"):
        gficf_amd.find_nn_sparse(np.zeros(5), 2)
    with pytest.raises(ValueError, match="needs a gene and a cell"):
        gficf_amd.find_nn_sparse(sp.csc_matrix((0, 5)), 2)
    rows = M.indices.copy()
    b = M.indptr[np.argmax(np.diff(M.indptr) >= 2)]
    rows[b], rows[b + 1] = rows[b + 1], rows[b]
    unsorted = sp.csc_matrix((M.data, rows, M.indptr), shape=M.shape)
    unsorted.has_sorted_indices = True                                    # a caller's promise that does not hold
    with pytest.raises(ValueError, match="strictly ascending"):
        gficf_amd.find_nn_sparse(unsorted, 5)
    rows[b + 1] = rows[b]
    twice = sp.csc_matrix((M.data, rows, M.indptr), shape=M.shape)
    twice.has_sorted_indices = True
    with pytest.raises(ValueError, match="strictly ascending"):
        gficf_amd.find_nn_sparse(twice, 5)
    for bad in (np.nan, np.inf, 1e39):                                    # 1e39 is finite in f64 and not in f32
        x = M.data.copy()
        x[3] = bad
        with pytest.raises(ValueError, match="finite as float32"):
            gficf_amd.find_nn_sparse(sp.csc_matrix((x, M.indices, M.indptr), shape=M.shape), 5)
    with pytest.raises(ValueError, match="q_begin"):
        gficf_amd.find_nn_sparse_range(M, 5, 3, 41)


def test_refusals_name_run_reduction_sparse():
    with pytest.raises(NotImplementedError, match="pca") as e:
        gficf_amd.runReduction({"gficf": None}, verbose=False)
    assert "runReductionSparse" in str(e.value)
    with pytest.raises(NotImplementedError, match="pca") as e:
        gficf_amd.runTsne({"gficf": None}, verbose=False)
    assert "runReductionSparse" in str(e.value)
    model = {"uwot": {"space": "gficf"}, "reduction": "tumap", "pca": None}
    with pytest.raises(NotImplementedError, match="runReductionSparse"):
        gficf_amd.embedNewCells(model, sp.csc_matrix((5, 2)), verbose=False)


def test_run_reduction_sparse_keywords():
    data = {"gficf": so.case(30, 40, 0.3, 1)}
    with pytest.raises(ValueError, match="reduction must be one of"):
        gficf_amd.runReductionSparse(data, reduction="pca", verbose=False)
    with pytest.raises(TypeError, match=r"unknown argument\(s\) \['perplexity'\]"):
        gficf_amd.runReductionSparse(data, reduction="tumap", perplexity=5, verbose=False)
    with pytest.raises(TypeError, match=r"unknown argument\(s\) \['n_neighbors'\]"):
        gficf_amd.runReductionSparse(data, reduction="tsne", n_neighbors=5, verbose=False)
    with pytest.raises(ValueError, match="metric must be one of"):
        gficf_amd.runReductionSparse(data, metric="chebyshev", verbose=False)
    with pytest.raises(ValueError, match="needs data\\['gficf'\\]"):
        gficf_amd.runReductionSparse({}, verbose=False)
    assert "uwot" not in data and "embedded" not in data
