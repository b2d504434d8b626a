"""GPU: libgficf_tsne.so (perplexity graph, exact gradient, layout, the chained embedding) and its Python mirror.

Affinities.  Checked against their defining properties in f64 from the device's own beta and conditionals
(tests/helpers/tsne_cases.check_affinities): no second implementation in the loop.

Repulsion by counting.  All points at one position, and two sites at distance 1: every q is 1 or 1 / 2, so Z and rep are whole
numbers and quarters, derived and not computed.  v_rcp_f32 returns 1 for 1 and 1 / 2 for 2 exactly, the sums of such terms are
exact in f32 and in f64 at these sizes, so the answers are asserted EXACTLY.  A j counted twice or missed changes them by
whole units.  The sizes come from tsne_shape: below a tile, a tile +- 1, a row block +- 1, three row blocks x several slices
with a ragged last block and last slice.

Gradient against the f64 port.  Per row and coordinate |rep - rep_ref| <= (8 + T) 2^-24 sum_j q_ij^2 |y_i - y_j|: 8 roundings per
term and at most T sequential f32 additions, T = tsne_shape's tile (the tiles are added in f64); the same for Z and attr over
their own absolute sums, and the three combined for dC.  KL to 1e-6 relative (its sum runs in f64).

Layout against the port, the same P and the same float32 state given to both.  The yardstick is the port in f64.  On every
case the port was also run in f32 on the CPU: MEASURED below holds the largest coordinate deviation between its two runs and
the largest |coordinate| of the case (``python -m tests.helpers.tsne_cases`` prints the table).  The test constant is 8 x that
deviation, never below 64 * 2^-24 * the largest |coordinate|.  No vertex is excluded.  (The 1 500 random points have no structure
to hold the layout open: while the exaggeration lasts, attraction and repulsion are both linear in Y and the layout shrinks,
to 4e-31 at iteration 249, and opens again behind the switch; the window [249, 252) is checked at that scale.)

Quality.  Trustworthiness, 15-NN label purity and final KL of full runs against the port's own figures over the same seeds
(MEASURED_QUALITY, from the same command): with s = max - min of the port over its five seeds, no run may fall below the port's
minimum by more than s (trustworthiness, purity) or exceed its maximum KL by more than s."""
import numpy as np
import pytest

import gficf_amd
from gficf_amd import GficfError
from tests.helpers import tsne_cases as tc
from tests.helpers import tsne_np as tn
from tests.helpers import umap_cases as uc
from tests.helpers import umap_np as un

pytestmark = pytest.mark.gpu

# (|port f32 - port f64|, largest |coordinate|) per layout case (set, window of 1000 iterations)
MEASURED = {
    ("big", "0-1"): (1.682e-10, 7.235e-04),
    ("big", "0-3"): (7.719e-10, 1.251e-03),
    ("big", "249-252"): (1.034e-37, 3.954e-31),
    ("big", "600-603"): (4.246e-06, 3.015e+01),
    ("small", "0-1"): (1.489e-09, 6.307e-03),
    ("small", "0-3"): (4.086e-07, 1.510e+00),
    ("small", "249-252"): (1.010e-06, 7.993e+00),
    ("small", "600-603"): (5.795e-06, 4.325e+01),
}
# (trustworthiness, purity, KL) of the port in f64, seeds 1 - 5, 1000 iterations, perplexity 30, 1 200 x 20 blobs
MEASURED_QUALITY = [
    (0.98632, 1.00000, 0.73051),
    (0.98614, 1.00000, 0.73252),
    (0.98630, 1.00000, 0.72784),
    (0.98587, 1.00000, 0.73237),
    (0.98588, 1.00000, 0.73187),
]


def _nn(X, k):
    r = gficf_amd.find_nn(X, k, True, "euclidean")
    return r["idx"], r["dist"]


# ------------------------------------------------------------------------------------------------ affinities
@pytest.mark.parametrize("perplexity", tc.PERPLEXITIES)
@pytest.mark.parametrize("name", ["graph", "rand"])
def test_affinity_properties(name, perplexity):
    idx, dist = _nn(tc.affinity_input(name), 3 * perplexity + 1)
    P, beta, Pc = gficf_amd.tsne_affinities(idx, dist, perplexity, ret_cond=True)
    reach = tc.check_affinities(idx, dist, perplexity, P, beta, Pc)
    if name == "rand":
        assert reach.all()
    else:
        assert not reach[uc.GRAPH_CENTRE] and reach[:99].sum() >= 98
        K = 3 * perplexity
        assert (dist[uc.GRAPH_CENTRE, 1:] == dist[uc.GRAPH_CENTRE, 1]).all()        # the row of one distance
        own = idx[:, 1:] == np.arange(1, 301)[:, None]
        rows = [uc.GRAPH_CENTRE] + (list(range(99, 119)) if K < 20 else [])          # and, while K < 20, the identical points
        for i in rows:
            v = Pc[i][~own[i]]
            assert len(v) in (K, K - 1) and (v.view(np.uint32) == v.view(np.uint32)[0]).all()
            assert abs(float(v[0]) - 1.0 / len(v)) <= np.spacing(np.float32(1.0 / len(v)))
    P2, beta2, Pc2 = gficf_amd.tsne_affinities(idx, dist, perplexity, ret_cond=True)
    assert tc.same_bits(P, P2) and np.array_equal(beta, beta2) and np.array_equal(Pc, Pc2)
    assert tc.same_bits(P, gficf_amd.tsne_affinities(idx, dist, perplexity)[0])


def test_affinity_deferred_errors():
    X = tc.affinity_input("rand")
    idx, dist = _nn(X, 16)
    good = gficf_amd.tsne_affinities(idx, dist, 5)[0]
    for v in (np.nan, np.inf):
        d = dist.copy()
        d[9, 3] = v
        with pytest.raises(GficfError) as e:
            gficf_amd.tsne_affinities(idx, d, 5)
        assert e.value.status == "GFICF_ERR_BAD_VALUE"
    for v in (len(X) + 1, 0):
        bad = idx.copy()
        bad[7, 2] = v
        with pytest.raises(GficfError) as e:
            gficf_amd.tsne_affinities(bad, dist, 5)
        assert e.value.status == "GFICF_ERR_BAD_ID"
    assert tc.same_bits(good, gficf_amd.tsne_affinities(idx, dist, 5)[0])             # and nothing else happened


# ------------------------------------------------------------------------------------------------ repulsion by counting
def _sizes():
    return tc.counting_sizes(gficf_amd.tsne_shape(1000))


@pytest.mark.parametrize("which", range(6))
def test_repulsion_by_counting(which):
    N = _sizes()[which]
    P = tc.ring_graph(N)
    # (a) every point at one position
    g = gficf_amd.tsne_gradient(P, np.tile(np.float32([0.75, -1.5]), (N, 1)), 3.0)
    assert g["Z"] == float(N * (N - 1))
    assert (g["rep"] == 0).all() and (g["grad"] == 0).all()
    p = float(np.float32(1.0 / N))                                                     # the stored value of P
    assert abs(g["kl"] - N * p * np.log(p * N * (N - 1.0))) <= 1e-12 * np.log(N)
    # (b) two sites at distance 1
    Y, Z, rep = tc.two_sites(N)
    g = gficf_amd.tsne_gradient(P, Y)
    assert g["Z"] == Z
    assert np.array_equal(g["rep"].astype(np.float64), rep)


def test_counting_sizes_cover_the_shape():
    sizes = _sizes()
    s = [gficf_amd.tsne_shape(n) for n in sizes]
    tile, rpb = s[0]["tile"], s[0]["rows_per_block"]
    assert len(sizes) == 6 and sizes[0] < tile and tile - 1 in sizes and tile + 1 in sizes and rpb - 1 in sizes and rpb + 1 in sizes
    assert -(-sizes[-1] // rpb) >= 3 and s[-1]["slices"] >= 2 and sizes[-1] % rpb and sizes[-1] % tile and sizes[-1] <= 3000
    assert s[0]["slices"] == 1 and s[2]["slices"] == 2


# ------------------------------------------------------------------------------------------------ gradient against the f64 port
@pytest.fixture(scope="module")
def big_p():
    idx, dist = _nn(tc.layout_points("big"), 91)
    return gficf_amd.tsne_affinities(idx, dist, 30)[0]


@pytest.mark.parametrize("scale,x", [(1e-4, 12.0), (10.0, 1.0)])
def test_gradient_against_the_port(big_p, scale, x):
    N = tc.GRADIENT_N
    Y = (np.random.default_rng(8).standard_normal((N, 2)) * scale).astype(np.float32)
    T = gficf_amd.tsne_shape(N)["tile"]
    eps = (8 + T) * 2.0 ** -24
    ref = tn.gradient(big_p, Y, x, np.float64, sums=True)
    got = gficf_amd.tsne_gradient(big_p, Y, x)
    worst = {
        "rep": float((np.abs(got["rep"] - ref["rep"]) / (eps * ref["rep_abs"])).max()),
        "Z": abs(got["Z"] - ref["Z"]) / (eps * ref["Z_abs"]),
        "dC": float((np.abs(got["grad"] - ref["grad"])
                     / (eps * (x * ref["attr_abs"] + ref["rep_abs"] / ref["Z"] + np.abs(ref["rep"]) / ref["Z"]))).max()),
        "kl": abs(got["kl"] - ref["kl"]) / (1e-6 * abs(ref["kl"])),
    }
    print(f"gradient at scale {scale:g}: error / bound =", worst)
    assert all(v <= 1.0 for v in worst.values()), worst
    again = gficf_amd.tsne_gradient(big_p, Y, x)
    assert all(np.array_equal(got[k], again[k]) for k in got)


def test_gradient_deferred_errors():
    N = 300
    P = tc.ring_graph(N)
    Y = np.random.default_rng(2).standard_normal((N, 2)).astype(np.float32)
    good = gficf_amd.tsne_gradient(P, Y)
    ptr = P.indptr.astype(np.int64).copy()
    ptr[5] = ptr[4] - 1                                                                # a row pointer that decreases
    with pytest.raises(GficfError) as e:
        gficf_amd.tsne_gradient((ptr, P.indices, P.data), Y)
    assert e.value.status == "GFICF_ERR_BAD_CSC"
    col = P.indices.copy()
    col[17] = N
    with pytest.raises(GficfError) as e:
        gficf_amd.tsne_layout((P.indptr, col, P.data), Y, 10)
    assert e.value.status == "GFICF_ERR_BAD_ID"
    bad = Y.copy()
    bad[3, 1] = np.nan
    with pytest.raises(GficfError) as e:
        gficf_amd.tsne_layout(P, bad, 10)
    assert e.value.status == "GFICF_ERR_BAD_VALUE"
    with pytest.raises(GficfError) as e:
        gficf_amd.tsne_layout(P, Y, 10, iter_begin=5, iter_end=11)
    assert e.value.status == "GFICF_ERR_INVALID_ARG"
    again = gficf_amd.tsne_gradient(P, Y)
    assert all(np.array_equal(good[k], again[k]) for k in good)                        # and nothing else happened


# ------------------------------------------------------------------------------------------------ layout against the port
def _device_window(name, window):
    lo, hi = tc.WINDOWS[window]
    Y, uY, gains = tc.state(name, lo)
    return gficf_amd.tsne_layout(tc.layout_graph(name), Y, tc.LAYOUT_ITER, lo, hi, uY, gains, ret_state=True)


@pytest.mark.parametrize("name,window", tc.layout_cases())
def test_layout_against_the_port(name, window):
    got = _device_window(name, window)
    ref = tc.port_window(name, window, np.float64)
    measured, top = MEASURED[(name, window)]
    tol = tc.tolerance(measured, top)
    dev = float(np.abs(got[0].astype(np.float64) - ref[0]).max())
    print(f"layout {name} {window}: deviation {dev:.3e}, tolerance {tol:.3e}, largest coordinate {np.abs(ref[0]).max():.3e}")
    assert all(a.dtype == np.float32 and a.shape == ref[0].shape and np.isfinite(a).all() for a in got)
    assert dev <= tol
    assert np.abs(got[0].astype(np.float64).mean(axis=0)).max() <= 2.0 ** -20 * np.abs(got[0]).max()
    assert (got[2] >= 0.01).all()


def test_layout_split_repeat_and_means():
    P = tc.layout_graph("big")
    Y0 = tc.state("big", 0)[0]
    kw = dict(stop_lying_iter=5, mom_switch_iter=9, ret_state=True)                    # both switches inside the run
    whole = gficf_amd.tsne_layout(P, Y0, 20, **kw)
    a = gficf_amd.tsne_layout(P, Y0, 20, 0, 7, **kw)
    b = gficf_amd.tsne_layout(P, a[0], 20, 7, 20, a[1], a[2], **kw)
    again = gficf_amd.tsne_layout(P, Y0, 20, **kw)
    for w, s, r in zip(whole, b, again):
        assert np.array_equal(w.view(np.uint32), s.view(np.uint32)) and np.array_equal(w.view(np.uint32), r.view(np.uint32))
    for Y in (whole[0], a[0]):
        assert np.abs(Y.astype(np.float64).mean(axis=0)).max() <= 2.0 ** -20 * np.abs(Y).max()
    assert not np.array_equal(whole[0], a[0]) and (whole[2] != 1).any()
    none = gficf_amd.tsne_layout(P, Y0, 20, 4, 4, ret_state=True)                      # an empty window touches nothing
    assert np.array_equal(none[0], Y0) and (none[1] == 0).all() and (none[2] == 1).all()
    Y, kl = gficf_amd.tsne_layout(P, Y0, 20, ret_kl=True, stop_lying_iter=5, mom_switch_iter=9)
    assert np.array_equal(Y, whole[0]) and kl == gficf_amd.tsne_gradient(P, Y)["kl"]


# ------------------------------------------------------------------------------------------------ quality of full runs
@pytest.mark.parametrize("seed", tc.QUALITY_SEEDS)
def test_quality_of_full_runs(seed):
    X, labels, cells = uc.quality_input()
    r = gficf_amd.Rtsne(cells, perplexity=tc.QUALITY_PERPLEXITY, max_iter=tc.QUALITY_ITER, seed=seed)
    t, pur = un.quality(X, r["Y"], labels)
    port = np.array(MEASURED_QUALITY)
    lo, hi = port.min(axis=0), port.max(axis=0)
    s = hi - lo
    print(f"seed {seed}: trustworthiness {t:.5f}, purity {pur:.5f}, KL {r['costs']:.5f}; port min {lo}, max {hi}")
    assert t >= lo[0] - s[0]
    assert pur >= lo[1] - s[1]
    assert r["costs"] <= hi[2] + s[2]


# ------------------------------------------------------------------------------------------------ the chain and the mirror
def test_host_chain_equals_the_stages():
    X = tc.layout_points("small")
    r = gficf_amd.Rtsne(X, perplexity=5, max_iter=30, normalize=False, seed=9, ret_P=True, ret_nn=True)
    idx, dist = _nn(X, 16)
    assert np.array_equal(r["nn"]["idx"], idx) and np.array_equal(r["nn"]["dist"], dist)
    P = gficf_amd.tsne_affinities(idx, dist, 5)[0]
    assert tc.same_bits(r["P"], P)
    Y, kl = gficf_amd.tsne_layout(P, tn.initial(len(X), 9), 30, ret_kl=True)
    assert r["Y"].dtype == np.float64 and np.array_equal(r["Y"], Y.astype(np.float64)) and r["costs"] == kl
    assert r["N"] == len(X) and r["perplexity"] == 5 and r["theta"] == 0.5 and r["max_iter"] == 30 and r["eta"] == 200
    n = gficf_amd.Rtsne(X, perplexity=5, max_iter=30, seed=9)                           # normalize_input, on the host
    m = gficf_amd.Rtsne(tn.normalize_input(X), perplexity=5, max_iter=30, normalize=False, seed=9, theta=0.0)
    assert np.array_equal(n["Y"], m["Y"]) and not np.array_equal(n["Y"], r["Y"]) and n["P"] is None and n["nn"] is None


def test_run_tsne_and_the_defaults_with_an_initial_y():
    cells = np.random.default_rng(6).standard_normal((300, 5))
    data = gficf_amd.runTsne({"pca": {"cells": cells}}, perplexity=10, max_iter=50, verbose=False)
    emb = np.asarray(data["embedded"])
    assert list(data["embedded"].columns) == ["X", "Y"] and emb.shape == (300, 2) and np.isfinite(emb).all()
    assert data["reduction"] == "tsne" and data["uwot"] is None and data["tsne"]["stop_lying_iter"] == 250
    assert np.array_equal(emb, gficf_amd.Rtsne(cells, perplexity=10, max_iter=50)["Y"])
    data = gficf_amd.clustcells(data, from_embedded=True, verbose=False)
    assert len(data["cluster"]) == 300
    with pytest.raises(NotImplementedError, match="tsne"):
        gficf_amd.embedNewCells(data, None, verbose=False)
    given = gficf_amd.Rtsne(cells, perplexity=10, max_iter=20, Y_init=emb)
    assert given["stop_lying_iter"] == 0 and given["mom_switch_iter"] == 0
    zero = gficf_amd.Rtsne(cells, perplexity=10, max_iter=20, Y_init=emb, stop_lying_iter=0, mom_switch_iter=0)
    late = gficf_amd.Rtsne(cells, perplexity=10, max_iter=20, Y_init=emb, stop_lying_iter=250, mom_switch_iter=250)
    assert np.array_equal(given["Y"], zero["Y"]) and not np.array_equal(given["Y"], late["Y"])
