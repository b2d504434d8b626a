"""No GPU: the header and loader of libgficf_transform.so, the numpy port (tests/helpers/transform_np.py) against the statements
of include/gficf_transform.h (the checks tests/test_transform_gpu.py applies to the library), the vote's tie rule, and the
argument handling and table bookkeeping of embedNewCells / classify_cells (everything decided before the first library call)."""
import os
import re

import numpy as np
import pandas as pd
import pytest

import gficf_amd
from gficf_amd import _transform_lib, _umap_lib
from gficf_amd.api import _append_predicted
from tests.helpers import transform_cases as tc
from tests.helpers import transform_np as tn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ ABI
def test_header_and_loader_name_the_same_entries():
    text = open(os.path.join(ROOT, "include", "gficf_transform.h")).read()
    body = text[text.index("extern \"C\""):]
    declared = set(re.findall(r"\b(gficf_transform_\w+)\s*\(", body))
    assert declared == set(_transform_lib.SIGNATURES)
    assert "#define GFICF_TRANSFORM_ABI_VERSION 1" in text and _transform_lib.ABI_VERSION == 1
    core = open(os.path.join(ROOT, "include", "gficf_hip.h")).read()
    assert re.search(r"#define\s+GFICF_HIP_ABI_VERSION\s+7\b", core)
    umap = open(os.path.join(ROOT, "include", "gficf_umap.h")).read()
    assert "#define GFICF_UMAP_ABI_VERSION 1" in umap and _umap_lib.ABI_VERSION == 1


def test_header_lists_the_differences():
    text = open(os.path.join(ROOT, "include", "gficf_transform.h")).read()
    for phrase in ("row's own mean", "row's own largest membership", "one attraction", "class::knn"):
        assert phrase in text, phrase


# ------------------------------------------------------------------------------------------------ the port's memberships
@pytest.mark.parametrize("k", tc.MEMBERSHIP_KS)
@pytest.mark.parametrize("lc", tc.MEMBERSHIP_LCS + (3.0,))
def test_port_memberships(k, lc):
    idx, dist, _ = tc.membership_table(k)
    sigma, rho, W = tn.memberships(dist, lc)
    S = tc.check_memberships(dist, sigma, rho, W, lc)
    d = dist.astype(np.float64)
    inactive = sigma.astype(np.float64) > 1e-3 * d.mean(axis=1) * 1.001            # the floor does not bind
    solvable = inactive & ((np.maximum(d - rho[:, None], 0) > 0).sum(axis=1) > 0) & (sigma > 1e-30)
    assert solvable.sum() > 200 or k == 2                                           # (k = 2 beyond local_connectivity 2: rho is the row's largest distance)
    assert np.abs(S[solvable] - np.log2(k)).max(initial=0.0) < 1e-4
    if lc == 1.0:
        assert (rho == 0).all()                                                     # what umap-learn's and uwot's transform do
    if lc == 2.0:
        assert np.array_equal(np.delete(rho, tc.ROW_ZERO), np.delete(dist[:, 0], tc.ROW_ZERO)) and rho[tc.ROW_ZERO] == 0
    if lc == 3.0 and k >= 3:
        rows = [i for i in range(len(dist)) if i not in (tc.ROW_EQUAL, tc.ROW_ZERO)]
        assert np.array_equal(rho[rows], dist[rows, 1])                             # distinct positive distances: nz[f - 1], f = 2
    if lc == 1.5:
        rows = np.delete(np.arange(len(dist)), tc.ROW_ZERO)
        assert np.allclose(rho[rows], 0.5 * dist[rows, 0], rtol=1e-6)
    assert (W[tc.ROW_ZERO] == 1).all() and np.ptp(W[tc.ROW_EQUAL]) == 0


def test_port_init_is_the_weighted_mean_and_falls_back_to_the_plain_one():
    idx, W, Yt, _ = tc.layout_case("rand")
    W = W.copy()
    W[3] = 0.0
    Y0 = tn.init_positions(idx, W, Yt)
    w64, y64 = W.astype(np.float64), Yt.astype(np.float64)[idx - 1]
    with np.errstate(invalid="ignore"):
        want = (w64[:, :, None] * y64).sum(1) / w64.sum(1)[:, None]
    want[3] = y64[3].mean(0)
    assert np.abs(Y0 - want).max() <= 2 * (idx.shape[1] + 2) * 2.0 ** -24 * np.abs(Yt).max()


# ------------------------------------------------------------------------------------------------ the port's layout
def _lay(**kw):
    idx, W, Yt, Y0 = tc.layout_case("rand")
    args = dict(n_epochs=20, seed=3)
    args.update(kw)
    return tn.layout(idx, W, Yt, args.pop("Y0", Y0), **args)


def test_port_layout_split_equals_whole():
    whole = _lay()
    half = _lay(epoch_begin=0, epoch_end=9)
    assert np.array_equal(_lay(Y0=half, epoch_begin=9, epoch_end=20), whole)
    assert not np.array_equal(whole, tc.layout_case("rand")[3])
    assert not np.array_equal(_lay(seed=4), whole)


def test_port_layout_halves_with_offsets_equal_the_whole():
    idx, W, Yt, Y0 = tc.layout_case("rand")
    whole = tn.layout(idx, W, Yt, Y0, 20, seed=3)
    lo = tn.layout(idx[:250], W[:250], Yt, Y0[:250], 20, seed=3, query_offset=0)
    hi = tn.layout(idx[250:], W[250:], Yt, Y0[250:], 20, seed=3, query_offset=250)
    assert np.array_equal(np.concatenate([lo, hi]), whole)
    assert not np.array_equal(tn.layout(idx[250:], W[250:], Yt, Y0[250:], 20, seed=3, query_offset=0), whole[250:])


def test_port_layout_epoch_zero_leaves_the_positions_untouched():
    Y0 = tc.layout_case("rand")[3]
    assert np.array_equal(_lay(epoch_begin=0, epoch_end=1), Y0)
    q = tn.row_schedule(tc.layout_case("rand")[1])
    assert q.max() == 2 ** 32 - 1 and (q.max(axis=1) == 2 ** 32 - 1).all()          # every row's own maximum: the row-local schedule
    assert not tn.due(q, 0).any() and tn.due(q, 1).any(axis=1).all()


def test_crafted_case_takes_the_zero_distance_branch():
    idx, W, Yt, Y0 = tc.layout_case("crafted")
    assert np.array_equal(Y0[tc.CRAFTED], Yt[idx[tc.CRAFTED, 0] - 1])               # the cells start on a trained neighbour
    lo, hi = tc.RANGES[tc.CRAFTED_EPOCH]
    assert hi == lo + 1 and tn.due(tn.row_schedule(W)[tc.CRAFTED, 0], lo).all()     # whose entry is due in the chosen epoch


# ------------------------------------------------------------------------------------------------ the exact cases are not vacuous
@pytest.mark.parametrize("k", tc.EXACT_KS)
def test_exact_inputs_follow_the_recipe_of_the_rand_case(k):
    idx, W, Yt, Y0 = tc.layout_case("rand", k)
    assert idx.shape == W.shape == (500, k) and Yt.shape == (1500, 2) and Y0.shape == (500, 2) and max(tc.EXACT_MS) == 500
    assert idx.min() >= 1 and idx.max() <= 1500 and W.dtype == Y0.dtype == Yt.dtype == np.float32
    assert (W >= 0).all() and (W.max(axis=1) > 0).all() and np.isfinite(Y0).all()
    ref = tc.layout_case("rand")
    lead = min(k, tc.LAYOUT_K)
    assert np.array_equal(idx[:, :lead], ref[0][:, :lead]) and np.array_equal(Yt, ref[2])      # the same points, the same plane
    if k == tc.EXACT_CRAFTED_K:
        cidx, cW, _, cY0 = tc.layout_case("crafted", k)
        assert np.array_equal(cidx, idx) and np.array_equal(cW, W)
        assert np.array_equal(cY0[tc.CRAFTED], Yt[idx[tc.CRAFTED, 0] - 1])          # the cells start on a trained neighbour
        for n in range(*tc.EXACT_WINDOW):
            assert tn.due(tn.row_schedule(W)[tc.CRAFTED, 0], n).all()               # whose entry is due in the tested epochs


@pytest.mark.parametrize("k", tc.EXACT_KS)
def test_schedule_reaches_every_kind_of_round(k):
    """In both tested epochs a due entry sits in the first lane slot of a round; in the last one where a row fills a round
    (k >= 8); in a ragged last round where there is one (k no multiple of 8).  Some round has nothing due at k = 9, 17 and 128.
    Up to k = 8 none can: a row's one round holds its largest membership, which is due in every epoch but the first.  At
    k = 16 none does: no membership of this input is below 0.35 of its row's largest, and eight of them never all rest."""
    W = tc.layout_case("rand", k)[1]
    for n in range(*tc.EXACT_WINDOW):
        c = tc.round_coverage(W, n)
        assert c["first"] and c["last"] == (k >= tc.GROUP) and c["ragged"] == (k % tc.GROUP != 0), (k, n, c)
        if k != 16:
            assert c["empty"] == (k > tc.GROUP), (k, n, c)
    assert any(tc.round_coverage(tc.layout_case("rand", kk)[1], tc.EXACT_WINDOW[0])["empty"] for kk in tc.EXACT_KS)


@pytest.mark.parametrize("case", tc.exact_cases(), ids=lambda c: "-".join(str(v) for v in c))
def test_exact_cases_tell_float32_from_float64(case):
    """Equality with the float32 port is a statement the float64 port would fail: the two differ on every case, and every cell
    moves (its largest membership is due in both epochs; a crafted cell, attracted at d2 == 0, by its other entries or samples)."""
    name, k, rate = case
    Y0 = tc.layout_case(name, k)[3]
    f32, f64 = tc.exact_port(name, k, rate, np.float32), tc.exact_port(name, k, rate, np.float64)
    dev = float(np.abs(f32.astype(np.float64) - f64).max())
    print(f"{case}: {len(f32)} cells, |port f32 - port f64| = {dev:.3e}")
    assert f32.dtype == np.float32 and f32.shape == Y0.shape and np.isfinite(f32).all()
    assert dev > 0 and not np.array_equal(f32, f64.astype(np.float32))              # not even after rounding
    moved = (f32 != Y0).any(axis=1)
    if name == "crafted" and rate == 0:
        assert moved[:tc.CRAFTED.start].all() and moved[tc.CRAFTED.stop:].all() and moved[tc.CRAFTED].sum() > 40
    else:
        assert moved.all()


@pytest.mark.parametrize("k", tc.EXACT_KS)
def test_port_cell_depends_on_its_row_and_offset_only(k):
    """What lets the GPU tests compare M cells with the first M rows of one run of the port."""
    idx, W, Yt, Y0 = tc.layout_case("rand", k)
    whole = tc.exact_port("rand", k, 7)
    for M in tc.EXACT_MS[:-1]:
        assert np.array_equal(tn.layout(idx[:M], W[:M], Yt, Y0[:M], tc.LAYOUT_EPOCHS, **tc.exact_kw(7)), whole[:M])
    first, off = tc.EXACT_OFFSETS[0]
    assert np.array_equal(tc.exact_port("rand", k, 7, first=first, query_offset=off), whole[first:])
    first, off = tc.EXACT_OFFSETS[1]
    assert not np.array_equal(tc.exact_port("rand", k, 7, first=first, query_offset=off), whole)


@pytest.mark.parametrize("k", tc.INIT_KS)
def test_init_case_holds_zero_memberships_and_a_row_of_nothing_else(k):
    idx, W, Yt = tc.init_case(k)
    assert idx.shape == W.shape == (300, k) and idx.min() >= 1 and idx.max() <= len(Yt) == 400
    assert (W[tc.INIT_ZERO_ROW] == 0).all() and (W == 0).sum() > k and (W.sum(axis=1) > 0).sum() >= 250 and W.max() <= 1
    Y = tn.init_positions(idx, W, Yt)
    y64 = Yt.astype(np.float64)[idx - 1]
    assert np.abs(Y[tc.INIT_ZERO_ROW] - y64[tc.INIT_ZERO_ROW].mean(0)).max() <= 2 * (k + 2) * 2.0 ** -24 * 10
    assert np.isfinite(Y).all()


# ------------------------------------------------------------------------------------------------ vote
def test_vote_tie_rule_on_hand_made_rows():
    labels = np.array([0, 1, 2, 2, 1, 0, 3], dtype=np.int32)                        # training ids 1 .. 7
    rows = np.array([[1, 2, 3, 4, 5],        # labels 0 1 2 2 1: 1 and 2 tie at two votes, 1 is met first
                     [3, 2, 5, 4, 1],        # labels 2 1 1 2 0: the same tie, 2 is met first
                     [7, 1, 6, 2, 5],        # labels 3 0 0 1 1: 0 and 1 tie, 0 first; 3 comes first but has one vote
                     [7, 2, 1, 3, 4],        # labels 3 1 0 2 2: 2 wins outright, last in the row
                     [1, 2, 3, 7, 7]])       # labels 0 1 2 3 3: 3 wins outright
    assert tn.vote(rows, labels).tolist() == [1, 2, 0, 2, 3]
    assert tn.vote(rows[:, :1], labels).tolist() == [0, 2, 3, 3, 0]                 # k = 1: the nearest neighbour's label
    assert tn.vote(np.array([[1, 2, 3, 7]]), labels).tolist() == [0]                # all tie: the first


# ------------------------------------------------------------------------------------------------ the mirror
def _data(n=40, dim=5, with_model=True):
    rng = np.random.default_rng(1)
    data = {"pca": {"cells": rng.standard_normal((n, dim)), "genes": rng.standard_normal((30, dim))}, "w": np.ones(30),
            "genes": np.arange(30), "reduction": "tumap", "embedded": pd.DataFrame(rng.standard_normal((n, 2)), columns=["X", "Y"])}
    if with_model:
        data["uwot"] = {"embedding": np.asarray(data["embedded"]), "a": 1.0, "b": 1.0, "n_neighbors": 15, "metric": "euclidean",
                        "n_epochs": 200, "seed": 1}
    return data


def test_embed_new_cells_argument_checks():
    import scipy.sparse as sp

    x = sp.random(30, 6, 0.5, format="csc", random_state=0)
    with pytest.raises(ValueError, match=r"runReduction\(ret_model_pred=True\)"):
        gficf_amd.embedNewCells(_data(with_model=False), x, verbose=False)
    tsne = _data()
    tsne["reduction"] = "tsne"
    with pytest.raises(NotImplementedError, match="tsne"):
        gficf_amd.embedNewCells(tsne, x, verbose=False)
    with pytest.raises(TypeError, match="n_neighbours"):
        gficf_amd.embedNewCells(_data(), x, n_neighbours=10, verbose=False)
    with pytest.raises(TypeError, match="metric"):                                  # the model's, not an argument
        gficf_amd.embedNewCells(_data(), x, metric="cosine", verbose=False)
    with pytest.raises(ValueError, match="genes"):
        gficf_amd.embedNewCells(_data(), x, genes=np.arange(29), verbose=False)
    with pytest.raises(ValueError, match="rows"):
        gficf_amd.embedNewCells(_data(), x[:20], verbose=False)
    no_pca = _data()
    no_pca["pca"] = None
    with pytest.raises(ValueError, match="runPCA"):
        gficf_amd.embedNewCells(no_pca, x, verbose=False)


def test_umap_transform_and_search_argument_checks():
    d = _data()
    X = d["pca"]["cells"]
    with pytest.raises(ValueError, match="columns"):
        gficf_amd.find_nn_query(X, X[:, :4], 3)
    with pytest.raises(ValueError, match="metric"):
        gficf_amd.find_nn_query(X, X, 3, metric="hamming")
    with pytest.raises(ValueError, match="columns"):
        gficf_amd.umap_transform(X[:, :4], d["uwot"], X)
    with pytest.raises(ValueError, match="embedding"):
        gficf_amd.umap_transform(X, d["uwot"], X[:30])
    with pytest.raises(ValueError, match="init"):
        gficf_amd.umap_transform(X[:7], d["uwot"], X, init="spectral")
    with pytest.raises(ValueError, match="init"):
        gficf_amd.umap_transform(X[:7], d["uwot"], X, init=np.zeros((6, 2)))
    with pytest.raises(ValueError, match="classes"):
        gficf_amd.knn_classify(X, X[:7], np.zeros(39))
    with pytest.raises(ValueError, match="metric"):
        gficf_amd.knn_classify(X, X[:7], np.zeros(40), metric="hamming")


def test_classify_cells_argument_checks():
    with pytest.raises(ValueError, match="Please embed first new cells!"):
        gficf_amd.classify_cells(_data(), np.zeros(40))
    with pytest.raises(ValueError, match="Please embed first new cells!"):
        gficf_amd.classify_cells({"embedded": None}, np.zeros(40))
    with pytest.raises(ValueError, match="method"):
        gficf_amd.classify_cells(_data(), np.zeros(40), method="tsne")


def test_table_bookkeeping_on_a_stub_embedding():
    emb = pd.DataFrame({"X": [0.0, 1.0, 2.0], "Y": [3.0, 4.0, 5.0], "cluster": ["1", "2", "1"]})
    new = np.array([[9.0, 8.0], [7.0, 6.0]])
    out = _append_predicted(emb, new)
    assert list(out.columns) == ["X", "Y", "cluster", "predicted"] and len(out) == 5
    assert out["predicted"].tolist() == ["NO", "NO", "NO", "YES", "YES"]
    assert isinstance(out["predicted"].dtype, pd.CategoricalDtype) and list(out["predicted"].cat.categories) == ["NO", "YES"]
    assert out["cluster"].tolist()[:3] == ["1", "2", "1"] and out["cluster"][3:].isna().all()
    assert np.array_equal(np.asarray(out[["X", "Y"]])[3:], new) and np.array_equal(np.asarray(out[["X", "Y"]])[:3], np.asarray(emb[["X", "Y"]]))
    assert "predicted" not in emb.columns                                           # the caller's table is not touched
    again = _append_predicted(out, new[:1])                                         # a second batch: the first one keeps its YES
    assert again["predicted"].tolist() == ["NO", "NO", "NO", "YES", "YES", "YES"] and list(again.columns) == list(out.columns)
    plain = _append_predicted(pd.DataFrame(np.zeros((2, 2)), columns=["X", "Y"]), new)
    assert list(plain.columns) == ["X", "Y", "predicted"] and plain["predicted"].tolist() == ["NO", "NO", "YES", "YES"]
