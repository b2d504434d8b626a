"""No GPU: the numpy port of libgficf_tsne.so (tests/helpers/tsne_np.py) against what defines it (its gradient is the gradient of
its own KL divergence, over 4; its affinities have the properties tests/test_tsne_gpu.py asks of the library; its iterations
are stateless and switch where include/gficf_tsne.h says), the header against the loader, and the argument handling of the
Python mirror (everything it decides before the first call into the library)."""
import os
import re

import numpy as np
import pytest

import gficf_amd
from gficf_amd import GficfError, _tsne_lib
from tests.helpers import tsne_cases as tc
from tests.helpers import tsne_np as tn
from tests.helpers import umap_np as un

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ ABI
def test_header_and_loader_name_the_same_entries():
    text = open(os.path.join(ROOT, "include", "gficf_tsne.h")).read()
    body = re.sub(r"/\*.*?\*/", "", text[text.index("extern \"C\""):], flags=re.S)
    declared = {m.group(1): m.group(2) for m in re.finditer(r"\b(gficf_tsne_\w+)\s*\(([^)]*)\)\s*;", body)}
    assert set(declared) == set(_tsne_lib.SIGNATURES)
    for name, args in declared.items():
        n = 0 if args.strip() == "void" else args.count(",") + 1
        assert n == len(_tsne_lib.SIGNATURES[name][1]), name
    assert "#define GFICF_TSNE_ABI_VERSION 1" in text and _tsne_lib.ABI_VERSION == 1
    assert re.search(r"#define\s+GFICF_TSNE_TILE\s+%d\b" % _tsne_lib.TILE, text)
    core = open(os.path.join(ROOT, "include", "gficf_hip.h")).read()
    assert re.search(r"#define\s+GFICF_HIP_ABI_VERSION\s+7\b", core)


def test_shape_is_a_host_query_of_n_alone():
    for n in (1, 127, 128, 129, 1500, 54000, 200000):
        s = gficf_amd.tsne_shape(n)
        assert s == gficf_amd.tsne_shape(n) and s["tile"] == _tsne_lib.TILE and s["rows_per_block"] % 64 == 0
        tiles = -(-n // s["tile"])
        assert 1 <= s["slices"] <= tiles                            # no slice without a tile
        per = -(-tiles // s["slices"])
        assert (s["slices"] - 1) * per < tiles <= s["slices"] * per
    sizes = tc.counting_sizes(gficf_amd.tsne_shape(1000))
    big = gficf_amd.tsne_shape(sizes[-1])
    assert sizes[-1] <= 3000 and -(-sizes[-1] // big["rows_per_block"]) >= 3 and big["slices"] >= 2
    assert sizes[-1] % big["rows_per_block"] and sizes[-1] % big["tile"]
    with pytest.raises(GficfError) as e:
        gficf_amd.tsne_shape(0)
    assert e.value.status == "GFICF_ERR_INVALID_ARG"


# ------------------------------------------------------------------------------------------------ the port: gradient
@pytest.fixture(scope="module")
def sixty():
    X = np.random.default_rng(3).standard_normal((60, 5))
    idx, dist = un.exact_knn(X, 16)
    P = tn.affinities(idx, dist, 5)[0]
    return P, np.random.default_rng(4).standard_normal((60, 2))


def test_port_gradient_is_a_quarter_of_the_gradient_of_its_kl(sixty):
    P, Y = sixty
    g = tn.gradient(P, Y)["grad"]
    h = 1e-5
    num = np.zeros_like(Y)
    for i in range(60):
        for c in range(2):
            up, dn = Y.copy(), Y.copy()
            up[i, c] += h
            dn[i, c] -= h
            num[i, c] = (tn.kl_divergence(P, up) - tn.kl_divergence(P, dn)) / (2 * h) / 4.0
    # central difference: the error is h^2 / 6 times a third derivative of order 1, and 2^-53 KL / h of rounding
    assert np.abs(num - g).max() < 1e-8 and np.abs(g).max() > 1e-4
    gx = tn.gradient(P, Y, 12.0)
    assert np.allclose(gx["grad"], 12.0 * gx["attr"] - gx["rep"] / gx["Z"], rtol=0, atol=1e-15)     # exaggeration: the attractive sum only


def test_port_gradient_sums_and_precisions(sixty):
    P, Y = sixty
    g64, g32 = tn.gradient(P, Y, sums=True), tn.gradient(P, Y, dtype=np.float32)
    assert g32["grad"].dtype == np.float32 and g64["grad"].dtype == np.float64
    assert (np.abs(g64["rep"]) <= g64["rep_abs"] * (1 + 1e-12)).all() and (np.abs(g64["attr"]) <= g64["attr_abs"] * (1 + 1e-12)).all()
    assert np.abs(g32["grad"] - g64["grad"]).max() < 1e-6 and abs(g32["kl"] - g64["kl"]) < 1e-5


# ------------------------------------------------------------------------------------------------ the port: affinities
@pytest.mark.parametrize("perplexity", tc.PERPLEXITIES)
@pytest.mark.parametrize("name", ["graph", "rand"])
def test_port_affinity_properties(name, perplexity):
    idx, dist = un.exact_knn(tc.affinity_input(name), 3 * perplexity + 1)
    P, beta, Pc = tn.affinities(idx, dist, perplexity)
    reach = tc.check_affinities(idx, dist, perplexity, P, beta, Pc)
    if name == "rand":
        assert reach.all()
    else:
        # the row of one distance; the random points (one of which has the 20 identical points as its nearest: unreachable below 20)
        assert not reach[119] and reach[:99].sum() >= 98


# ------------------------------------------------------------------------------------------------ the port: iterations
@pytest.fixture(scope="module")
def small():
    return tc.layout_graph("small"), tn.initial(257, 3)


def test_port_split_equals_whole(small):
    P, Y0 = small
    kw = dict(stop_lying_iter=5, mom_switch_iter=9)
    whole = tn.layout(P, Y0, 20, **kw)
    a = tn.layout(P, Y0, 20, 0, 7, **kw)
    b = tn.layout(P, a[0], 20, 7, 20, a[1], a[2], **kw)
    for x, y in zip(whole, b):
        assert np.array_equal(x, y)
    assert not np.array_equal(whole[0], Y0.astype(np.float32)) and (whole[2] != 1).any() and (whole[1] != 0).any()
    assert np.abs(whole[0].astype(np.float64).mean(axis=0)).max() <= 2.0 ** -20 * np.abs(whole[0]).max()


def test_port_switches_where_the_contract_says(small):
    P, Y0 = small
    st = (Y0.astype(np.float32), np.zeros((257, 2), np.float32), np.ones((257, 2), np.float32))
    for n in range(8):
        nxt = tn.layout(P, st[0], 20, n, n + 1, st[1], st[2], stop_lying_iter=3, mom_switch_iter=5)
        x, mu = (12.0 if n < 3 else 1.0), (0.5 if n < 5 else 0.8)
        assert tn.schedule(n, 3, 5, 0.5, 0.8, 12.0) == (x, mu)
        by_hand = tn.step(P, *st, x, mu, 200.0, np.float32)
        other = tn.step(P, *st, 1.0 if n < 3 else 12.0, mu, 200.0, np.float32)
        for a, b in zip(nxt, by_hand):
            assert np.array_equal(a, b), n
        assert not np.array_equal(nxt[0], other[0]), n              # and the exaggeration does matter
        st = nxt


# ------------------------------------------------------------------------------------------------ the mirror's argument handling
def _x(n=100, dim=5):
    return np.random.default_rng(1).standard_normal((n, dim))


def test_rtsne_argument_checks():
    with pytest.raises(ValueError, match="dims"):
        gficf_amd.Rtsne(_x(), dims=3)
    with pytest.raises(ValueError, match="pca"):
        gficf_amd.Rtsne(_x(), pca=True)
    with pytest.raises(ValueError, match="perplexity is too large|too large for the number of samples"):
        gficf_amd.Rtsne(_x(90), perplexity=30)                      # N - 1 = 89 < 90
    with pytest.raises(ValueError, match="perplexity"):
        gficf_amd.Rtsne(_x(), perplexity=0)
    with pytest.raises(GficfError) as e:
        gficf_amd.Rtsne(_x(200), perplexity=43)
    assert e.value.status == "GFICF_ERR_UNSUPPORTED"
    with pytest.raises(ValueError, match="Y_init"):
        gficf_amd.Rtsne(_x(), perplexity=5, Y_init=np.zeros((99, 2)))
    with pytest.raises(ValueError, match="2-d"):
        gficf_amd.Rtsne(np.zeros(10))
    with pytest.raises(TypeError):
        gficf_amd.Rtsne(_x(), perplexty=5)


def test_run_tsne_argument_checks():
    data = {"pca": {"cells": _x()}}
    with pytest.raises(TypeError, match="perplexty"):
        gficf_amd.runTsne(data, perplexty=5, verbose=False)
    with pytest.raises(TypeError, match="dims"):
        gficf_amd.runTsne(data, dims=2, verbose=False)              # fixed by the reference's call
    with pytest.raises(NotImplementedError, match="pca"):
        gficf_amd.runTsne({"gficf": None}, verbose=False)
    with pytest.raises(ValueError, match="too large"):
        gficf_amd.runTsne({"pca": {"cells": _x(50)}}, verbose=False)
    assert "embedded" not in data and "reduction" not in data


def test_stage_argument_checks():
    idx, dist = un.exact_knn(_x(40), 16)
    with pytest.raises(ValueError, match="columns"):
        gficf_amd.tsne_affinities(idx, dist, perplexity=10)         # needs 31 columns
    with pytest.raises(ValueError, match="same shape"):
        gficf_amd.tsne_affinities(idx, dist[:, :5], perplexity=5)
    with pytest.raises(GficfError) as e:
        gficf_amd.tsne_affinities(np.ones((300, 130), np.int32), np.ones((300, 130)), perplexity=43)
    assert e.value.status == "GFICF_ERR_UNSUPPORTED"


def test_run_reduction_still_declines_tsne():
    data = {"pca": {"cells": _x(40)}}
    with pytest.raises(NotImplementedError, match="tsne") as e:
        gficf_amd.runReduction(data, reduction="tsne", verbose=False)
    assert "runTsne" in str(e.value)
    with pytest.raises(NotImplementedError, match="tsne") as e:
        gficf_amd.embedNewCells({"reduction": "tsne"}, None, verbose=False)
    assert "runTsne" in str(e.value)
