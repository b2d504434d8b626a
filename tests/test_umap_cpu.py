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


# ------------------------------------------------------------------------------------------------ the exact cases are not vacuous
def _check_shape_graph(P, lengths):
    assert P.dtype == np.float32 and np.array_equal(np.diff(P.indptr), lengths)
    for i in range(P.shape[0]):
        c = P.indices[P.indptr[i]:P.indptr[i + 1]]
        assert (np.diff(c) > 0).all() and not (c == i).any() and (len(c) == 0 or (c[0] >= 0 and c[-1] < P.shape[0])), i
    assert P.data.min() >= np.float32(0.05) and P.data.max() <= 1


def test_seams_has_the_row_lengths_it_claims():
    P, Y0 = uc.seams()
    length = np.diff(P.indptr)
    assert P.shape == (300, 300) and Y0.shape == (300, 2) and np.abs(Y0).max() <= 10
    assert tuple(length[:20]) == uc.SEAM_LENGTHS and length[20:].max() < 20
    assert {0, 1, 2, 7, 8, 9, 15, 16, 17, 24, 25, 63, 64, 65, 255, 256, 257, 258, 299} <= set(length.tolist())
    assert (length == 0).sum() >= 2 and (length > uc.HUB_LEN).sum() == 3
    _check_shape_graph(P, length)
    shared = np.arange(300)[uc.SEAM_SHARED]
    assert len(shared) == 30 and len(np.unique(Y0[shared], axis=0)) == 1 and len(np.unique(Y0, axis=0)) == 271
    for v in shared:                                                                # their rows name each other only
        assert np.isin(P.indices[P.indptr[v]:P.indptr[v + 1]], shared).all()


def test_many_hubs_has_more_hubs_than_hub_waves():
    P, Y0 = uc.many_hubs()
    length = np.diff(P.indptr)
    hubs = length[length > uc.HUB_LEN]
    assert P.shape == (1100, 1100) and len(hubs) == 1030 > uc.HUB_WAVES and (length <= uc.HUB_LEN).sum() == 70
    assert np.array_equal(hubs, 257 + np.arange(1030) % 44) and length[length <= uc.HUB_LEN].max() < 20
    assert 280_000 < P.nnz < 290_000
    assert P.nnz // uc.HUB_LEN + 1 >= 1030                                          # the hub list of the library holds them all
    _check_shape_graph(P, length)


@pytest.mark.parametrize("L,pad", uc.PADDED)
def test_padded_differs_from_its_plain_form_in_entries_that_are_never_due(L, pad):
    P, Y0, v = uc.padded(L, pad)
    Q, Y0q, vq = uc.padded(L, 0)
    assert v == vq == P.shape[0] - 1 and np.array_equal(Y0, Y0q)
    assert np.diff(P.indptr)[v] == L + pad > uc.HUB_LEN >= L == np.diff(Q.indptr)[v]      # the wave path against the group path
    assert np.diff(P.indptr)[:v].max() < 20
    n = Q.nnz
    assert P.nnz == n + pad and np.array_equal(P.indptr[:-1], Q.indptr[:-1])
    assert np.array_equal(P.indices[:n], Q.indices) and np.array_equal(P.data[:n].view(np.uint32), Q.data.view(np.uint32))
    assert (P.indices[n:] > P.indices[n - 1]).all() and (np.diff(P.indices[P.indptr[v]:]) > 0).all() and P.indices[-1] < v
    q = un.schedule(P.data)
    assert (q[n:] == 0).all() and np.array_equal(q[:n], un.schedule(Q.data))         # the padding: schedule word 0, the rest unchanged
    lo, hi = uc.WINDOWS[uc.PADDED_WINDOW]
    for e in range(lo, hi):
        assert un.due(q[P.indptr[v]:], e).sum() > 20                                # row v has work in every epoch of the window


def _windows_of(graph):
    return sorted({w for g, w, _ in uc.exact_cases() if g == graph})


@pytest.mark.parametrize("graph", ["seams", "many_hubs", "rand", "hub"])
def test_schedule_reaches_every_kind_of_round(graph):
    """In every epoch of every tested window beyond epoch 0: a due entry in the first and in the last lane slot of a round, one
    in a ragged last round, and a round without any; on both paths of the crafted graphs, on the group path of the two kNN
    graphs ("rand" has no hub, and the one hub of "hub" has few due entries: what the crafted graphs are for)."""
    P, _ = uc.exact_graph(graph)
    for w in _windows_of(graph):
        for n in range(*uc.WINDOWS[w]):
            if n == 0:
                assert not un.due(un.schedule(P.data), 0).any()
                continue
            cov = uc.round_coverage(P, n)
            for G in (uc.GROUP, uc.WAVE) if graph in ("seams", "many_hubs") else (uc.GROUP,):
                c = cov[G]
                assert c["rows"] > 0 and c["first"] and c["last"] and c["ragged"] and c["empty"], (graph, n, G, c)


def test_negative_samples_name_their_own_vertex():
    for graph, w, rate in uc.exact_cases():
        lo, hi = uc.WINDOWS[w]
        if graph in ("seams", "many_hubs") and rate >= 5 and lo > 0:
            P, _ = uc.exact_graph(graph)
            assert sum(uc.self_samples(P, n, rate) for n in range(lo, hi)) > 0, (graph, w, rate)


def test_seams_takes_the_zero_distance_branches_of_both_forces():
    for n in (100,):                                                                # the first epoch of both windows beyond epoch 0
        for rate in uc.SEAM_RATES:
            attractions, repulsions = uc.seams_zero_distance(n, rate)
            assert attractions >= 2 and (repulsions >= 1 or rate == 0), (rate, attractions, repulsions)


@pytest.mark.parametrize("case", uc.exact_cases(), ids=uc.exact_id)
def test_exact_cases_tell_float32_from_float64(case):
    """Equality with the float32 port is a statement the float64 port would fail: the two differ on every case, the sweep moves
    every vertex with a due entry towards a vertex that is somewhere else, and leaves every vertex without a due entry alone."""
    graph, w, rate = case
    P, Y0 = uc.exact_graph(graph)
    f32, f64 = uc.exact_port(graph, w, rate, np.float32), uc.exact_port(graph, w, rate, np.float64)
    start = np.asarray(Y0, dtype=np.float32)
    dev = float(np.abs(f32.astype(np.float64) - f64).max())
    print(f"{uc.exact_id(case)}: {len(f32)} vertices, |port f32 - port f64| = {dev:.3e}")
    assert f32.dtype == np.float32 and f32.shape == start.shape and np.isfinite(f32).all()
    lo, hi = uc.WINDOWS[w]
    q = un.schedule(P.data)
    rows, _ = uc.entry_rows(P)
    fire = np.zeros(P.nnz, dtype=bool)
    for n in range(lo, hi):
        fire |= un.due(q, n)
    idle = np.ones(len(start), dtype=bool)
    idle[rows[fire]] = False
    apart = fire & (start[rows] != start[P.indices]).any(axis=1)
    busy = np.zeros(len(start), dtype=bool)
    busy[rows[apart]] = True
    moved = (f32 != start).any(axis=1)
    assert not moved[idle].any() and moved[busy].all()
    if hi == 1:
        assert not fire.any() and np.array_equal(f32, start)                        # epoch 0: nothing is due, nothing to tell apart
    else:
        assert busy.sum() > len(start) // 2 and dev > 0
        assert not np.array_equal(f32, f64.astype(np.float32))                      # not even after rounding


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
