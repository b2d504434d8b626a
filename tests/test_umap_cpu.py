"""No GPU: the numpy port of libgficf_umap.so (tests/helpers/umap_np.py) against the defining properties of the fuzzy graph (the
checks tests/test_umap_gpu.py applies to the library), the integer schedule, find_ab_params against uwot's documented values,
and the argument handling of the Python mirror (everything it decides before the first call into the library)."""
import re
import os

import numpy as np
import pytest

import gficf_amd
from gficf_amd import _umap_lib
from gficf_amd.api import umap_init
from tests.helpers import umap_cases as uc
from tests.helpers import umap_np as un

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ ABI
def test_header_and_loader_name_the_same_entries():
    text = open(os.path.join(ROOT, "include", "gficf_umap.h")).read()
    body = text[text.index("extern \"C\""):]
    declared = set(re.findall(r"\b(gficf_umap_\w+)\s*\(", body))
    assert declared == set(_umap_lib.SIGNATURES)
    assert "#define GFICF_UMAP_ABI_VERSION 1" in text and _umap_lib.ABI_VERSION == 1
    core = open(os.path.join(ROOT, "include", "gficf_hip.h")).read()
    assert re.search(r"#define\s+GFICF_HIP_ABI_VERSION\s+7\b", core)


# ------------------------------------------------------------------------------------------------ the port's graph
@pytest.fixture(scope="module")
def graph_x():
    return uc.graph_input()


@pytest.mark.parametrize("k", uc.GRAPH_KS)
def test_port_graph_properties(graph_x, k):
    idx, dist = un.exact_knn(graph_x, k)
    sigma, rho, W = un.smooth_knn(idx, dist)
    P = un.symmetrise(idx, W)
    uc.check_graph(idx, dist, P, sigma, rho, W)
    assert (dist[uc.GRAPH_CENTRE, 1:] == dist[uc.GRAPH_CENTRE, 1]).all()           # the row of one distance
    if k <= 20:
        assert (rho[uc.GRAPH_BLOCK] == 0).all()                                     # the identical points
    if 3 <= k <= 20:                                                                # k - 1 ones exceed log2(k): the global-mean floor
        assert np.allclose(sigma[uc.GRAPH_BLOCK], 1e-3 * dist.astype(np.float64).mean(), rtol=1e-5)


@pytest.mark.parametrize("mix,lc", [(0.0, 1.0), (0.5, 1.0), (1.0, 1.5), (1.0, 2.0)])
def test_port_graph_mix_ratio_and_local_connectivity(graph_x, mix, lc):
    idx, dist = un.exact_knn(graph_x, 15)
    sigma, rho, W = un.smooth_knn(idx, dist, lc)
    P = un.symmetrise(idx, W, mix)
    uc.check_graph(idx, dist, P, sigma, rho, W, mix=mix, lc=lc)


def test_hub_table_gives_one_full_row():
    P, Y0 = uc.layout_graph("hub")
    assert P.shape == (2001, 2001) and np.diff(P.indptr).max() == 2000 and np.diff(P.indptr).min() >= 14


# ------------------------------------------------------------------------------------------------ find_ab_params
@pytest.mark.parametrize("min_dist,want", [(0.01, (1.8956, 0.8006)), (0.001, (1.929, 0.7915))])
def test_find_ab_params_gives_uwots_documented_values(min_dist, want):
    a, b = gficf_amd.find_ab_params(1, min_dist)
    assert abs(a - want[0]) < 1e-3 and abs(b - want[1]) < 1e-3


# ------------------------------------------------------------------------------------------------ schedule
@pytest.mark.parametrize("n_epochs", [1, 7, 200, 500])
def test_schedule_counts_and_pruning(n_epochs):
    rng = np.random.default_rng(n_epochs)
    w = np.concatenate([rng.random(500), [1.0, 1.0 / n_epochs, np.nextafter(1.0 / n_epochs, 0), 1e-9, 0.5]]).astype(np.float32)
    q = un.schedule(w)
    assert q.dtype == np.uint64 and q.max() == 2 ** 32 - 1
    fired = np.zeros(len(w), dtype=np.int64)
    for n in range(n_epochs):
        fired += un.due(q, n)
    assert np.array_equal(fired, (np.uint64(n_epochs) * q) >> np.uint64(32))
    below = w.astype(np.float64) < float(w.max()) / n_epochs
    assert (fired[below] == 0).all()                                                # uwot's pruning, and the only one
    assert fired[500] == n_epochs - 1                                               # wmax: every epoch but the first


def test_schedule_is_stateless():
    q = un.schedule(np.random.default_rng(0).random(100).astype(np.float32))
    a = [un.due(q, n) for n in range(50)]
    b = [un.due(q, n) for n in reversed(range(50))][::-1]
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_port_layout_split_equals_whole():
    P, Y0 = uc.layout_graph("rand")
    whole = un.layout(P, Y0, 20, seed=3)
    half = un.layout(P, Y0, 20, seed=3, epoch_begin=0, epoch_end=9)
    assert np.array_equal(un.layout(P, half, 20, seed=3, epoch_begin=9, epoch_end=20), whole)
    assert not np.array_equal(whole, np.asarray(Y0, dtype=np.float32))


# ------------------------------------------------------------------------------------------------ the mirror's argument handling
def _data(n=40, dim=5):
    return {"pca": {"cells": np.random.default_rng(1).standard_normal((n, dim))}}


def test_not_provided_paths_say_so():
    with pytest.raises(NotImplementedError, match="tsne"):
        gficf_amd.runReduction(_data(), reduction="tsne", verbose=False)
    with pytest.raises(NotImplementedError, match="spectral"):
        gficf_amd.runReduction(_data(), init="spectral", verbose=False)
    with pytest.raises(NotImplementedError, match="pca"):
        gficf_amd.runReduction({"gficf": None}, verbose=False)


def test_argument_checks():
    with pytest.raises(ValueError, match="reduction"):
        gficf_amd.runReduction(_data(), reduction="pca", verbose=False)
    with pytest.raises(TypeError, match="n_neighbours"):
        gficf_amd.runReduction(_data(), n_neighbours=10, verbose=False)
    with pytest.raises(ValueError, match="metric"):
        gficf_amd.runReduction(_data(), metric="hamming", verbose=False)
    with pytest.raises(ValueError, match="init"):
        gficf_amd.runReduction(_data(), init="laplacian", verbose=False)
    with pytest.raises(ValueError, match="init"):
        gficf_amd.runReduction(_data(), init=np.zeros((39, 2)), verbose=False)
    with pytest.raises(ValueError, match="two PCA components"):
        gficf_amd.runReduction(_data(dim=1), verbose=False)
    with pytest.raises(ValueError):
        gficf_amd.find_ab_params(0, 0.01)


def test_init_pca_scaling_and_noise():
    cells = np.random.default_rng(2).standard_normal((500, 6)) * 37.0
    Y = umap_init("pca", cells, 500, 9)
    base = cells[:, :2] * (10.0 / np.abs(cells[:, :2]).max())
    assert np.abs(base).max() == pytest.approx(10.0, abs=1e-12)
    noise = Y - base
    assert np.allclose(noise, np.random.default_rng(9).normal(0.0, 1e-4, size=(500, 2)), rtol=0, atol=1e-12)
    assert 5e-5 < noise.std() < 2e-4 and abs(np.abs(Y).max() - 10.0) < 1e-3
    assert np.array_equal(umap_init("pca", cells, 500, 9), Y) and not np.array_equal(umap_init("pca", cells, 500, 10), Y)


def test_init_random_and_given():
    Y = umap_init("random", None, 1000, 4)
    assert Y.shape == (1000, 2) and Y.min() >= -10 and Y.max() < 10 and Y.std() > 5
    given = np.arange(20.0).reshape(10, 2)
    assert np.array_equal(umap_init(given, None, 10, 0), given)
