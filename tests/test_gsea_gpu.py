"""GPU: gene-set enrichment (libgficf_gsea.so) against the NumPy oracle of tests/helpers/gsea_np.py.
Bar: ES, the permutations, the null table and pval bit for bit; NES within rtol nsim * 2^-52 (sums of at most nsim same-signed
f64 values in any order differ by at most (nsim - 1) * 2^-53 relative; the mean and the quotient add one rounding each) and
the same bits on every call."""
import numpy as np
import pytest

import gficf_amd
from gficf_amd import GficfError, _gsea_lib
from gficf_amd.api import _np_ptr, check, default_context
from tests.helpers import gsea_np as gs

pytestmark = pytest.mark.gpu

SEED = 180582
ES_G = [33, 63, 64, 65, 1000, 8225]


def _csr(sets):
    ptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    return ptr, np.concatenate([np.asarray(s, dtype=np.int32) for s in sets]).astype(np.int32)


def _stats(G, seed):
    """Three clusters: distinct values, all equal, a 60 % zero tail with some -0.0."""
    rng = np.random.default_rng(seed)
    S = np.empty((G, 3))
    S[:, 0] = rng.normal(size=G)
    S[:, 1] = 2.5
    S[:, 2] = np.abs(rng.normal(size=G))
    S[rng.random(G) < 0.6, 2] = 0.0
    S[rng.random(G) < 0.1, 2] = -0.0
    return S


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _perm_host(G, seed, j):
    out = np.full(G, -1, dtype=np.int32)
    check(_gsea_lib.load().gficf_gsea_permutation_host(default_context().handle, G, seed, j, _np_ptr(out)))
    return out


@pytest.mark.parametrize("G", ES_G)
def test_observed_es_bit_exact(G):
    rng = np.random.default_rng(G)
    S = _stats(G, G)
    o = gs.order_desc(S[:, 0])                               # sets placed by their positions in cluster 0
    sets = [[o[0]], [o[G // 2]], [o[G - 1]], o[:G - 1], o[1:], o[:min(20, G - 1)], o[G - min(20, G - 1):], o[30:min(35, G)], o[31:33],
            np.arange(G - 1)]
    for m in (2, 7, 15, min(64, G - 1), G // 2, G - 2):
        sets.append(rng.choice(G, m, replace=False))
    ptr, rows = _csr(sets)
    r = gficf_amd.gsea(S, ptr, rows, nsim=4, seed=SEED)
    assert r["tested"].all() and np.array_equal(r["size"], np.diff(ptr))
    want = np.array([[gs.es_of_set(gs.ranks(S[:, c])[s], G) for c in range(3)] for s in sets])
    assert _same_bits(r["es"], want), np.argwhere(r["es"] != want)
    lit = np.array([[gs.es_literal(S[:, c], s) for c in range(3)] for s in sets])
    assert _same_bits(r["es"], lit)
    assert r["es"][0, 0] == 1.0 and r["es"][2, 0] == -1.0 and r["es"][5, 0] == 1.0 and r["es"][6, 0] == -1.0
    assert r["es"][9, 1] == 1.0                              # all statistics equal: ties by row, rows 0 .. G - 2 lead


@pytest.mark.parametrize("G", ES_G)
def test_permutation_probe_equals_the_oracle(G):
    B = int(_gsea_lib.load().gficf_gsea_perm_batch(G, 1 << 20))
    nsim = 2 * B + 3
    for j in (0, 1, B - 1, B, nsim - 1):
        assert np.array_equal(_perm_host(G, SEED, j), gs.perm(G, SEED, j)), (G, j)
    assert np.array_equal(_perm_host(G, 7, 2 ** 32 - 1), gs.perm(G, 7, 2 ** 32 - 1))


@pytest.fixture(scope="module")
def null_runs():
    """(G, sizes) -> (device result with ret_null, the oracle's null), nsim one past a batch: computed once, left unchanged."""
    out = {}
    for G, sizes in ((65, (1, 15, 32, 64)), (8225, (15, 257, 4000))):
        nsim = int(_gsea_lib.load().gficf_gsea_perm_batch(G, 1 << 20)) + 1
        ptr, rows = _csr([np.arange(m) for m in sizes])
        S = np.random.default_rng(G).normal(size=(G, 1))
        out[G] = (sizes, nsim, gficf_amd.gsea(S, ptr, rows, nsim=nsim, seed=SEED, ret_null=True), gs.null(G, SEED, sizes, nsim))
    return out


@pytest.mark.parametrize("G", [65, 8225])
def test_null_table_bit_exact_across_a_batch_boundary(null_runs, G):
    sizes, nsim, r, want = null_runs[G]
    assert nsim == int(_gsea_lib.load().gficf_gsea_perm_batch(G, nsim)) + 1
    assert np.array_equal(r["sizes"], sizes) and r["null"].shape == (len(sizes), nsim)
    assert _same_bits(r["null"], want), np.argwhere(r["null"] != want)[:5]


def test_cut_invariance():
    G = 1000
    S = np.random.default_rng(1).normal(size=(G, 2))
    ptr, rows = _csr([np.arange(15), np.arange(40) + 100])
    a = gficf_amd.gsea(S, ptr, rows, nsim=250, seed=SEED, ret_null=True)
    b = gficf_amd.gsea(S, ptr, rows, nsim=100, seed=SEED, ret_null=True)
    assert _same_bits(a["null"][:, :100], b["null"])
    ptr2, rows2 = _csr([np.arange(7), np.arange(15), np.arange(40) + 100, np.arange(100) + 300, np.arange(999)])
    c = gficf_amd.gsea(S, ptr2, rows2, nsim=100, seed=SEED, ret_null=True)
    assert c["sizes"].tolist() == [7, 15, 40, 100, 999]
    assert _same_bits(c["null"][[1, 2]], b["null"])
    assert _same_bits(c["es"][[1, 2]], b["es"]) and _same_bits(c["pval"][[1, 2]], b["pval"]) and _same_bits(c["nes"][[1, 2]], b["nes"])
    d = gficf_amd.gsea(S, ptr, rows, nsim=100, seed=SEED + 1, ret_null=True)
    assert not np.array_equal(d["null"], b["null"]) and _same_bits(d["es"], b["es"])


def _check_against(r, w, nsim):
    """A device result against gsea_np's."""
    assert np.array_equal(r["tested"], w["tested"]) and np.array_equal(r["size"], w["size"])
    assert _same_bits(r["es"], w["es"])
    assert _same_bits(r["pval"], w["pval"]), np.abs(r["pval"] - w["pval"]).max()
    t = w["tested"]
    np.testing.assert_allclose(r["nes"][t], w["nes"][t], rtol=nsim * 2.0 ** -52, atol=0, equal_nan=True)
    for k in ("es", "nes", "pval"):
        assert (_bits(r[k][~t]) == 0).all(), k


def test_statistics_against_the_oracle():
    G, nsim = 1000, 300
    rng = np.random.default_rng(5)
    S = _stats(G, 5)
    sets = [rng.choice(G, int(m), replace=False) for m in rng.integers(5, 90, 40)]
    sets += [rng.choice(G, 20, replace=False) for _ in range(3)]                 # several pathways of one size
    sets.append(gs.order_desc(S[:, 0])[:30])                                     # ES = 1: the null's upper tail
    sets.append(gs.order_desc(S[:, 0])[-30:])                                    # ES = -1
    ptr, rows = _csr(sets)
    kw = dict(nsim=nsim, min_size=12, max_size=70, seed=SEED)
    r = gficf_amd.gsea(S, ptr, rows, ret_null=True, **kw)
    w = gs.gsea_np(S, ptr, rows, **kw)
    assert 0 < (~w["tested"]).sum() < len(sets) and (np.diff(ptr)[~w["tested"]] < 12).any() and (np.diff(ptr)[~w["tested"]] > 70).any()
    assert np.array_equal(r["sizes"], w["sizes"]) and _same_bits(r["null"], w["null"])
    _check_against(r, w, nsim)
    # the four counts, taken from what the device returned (its ES, its null), are the oracle's
    for p in np.flatnonzero(w["tested"]):
        for c in range(3):
            s = gs.stats_of(r["es"][p, c], r["null"][np.searchsorted(r["sizes"], r["size"][p])])
            for k in ("nGeEs", "nLeEs", "nGeZero", "nLeZero"):
                assert s[k] == w[k][p, c], (k, p, c)
            assert _bits(np.float64(s["pval"])) == _bits(r["pval"][p, c])
    assert w["pval"][-2, 0] == 1 / (1 + w["nGeZero"][-2, 0]) and w["pval"][-1, 0] == 1 / (1 + w["nLeZero"][-1, 0])
    again = gficf_amd.gsea(S, ptr, rows, **kw)
    for k in ("es", "nes", "pval"):
        assert _same_bits(again[k], r[k]), k
    # G - 1 caps the sizes whatever max_size says
    few = gficf_amd.gsea(S[:50], *_csr([np.arange(49), np.arange(50), np.arange(10)]), nsim=20, seed=SEED)
    assert few["tested"].tolist() == [True, False, True] and (few["es"][1] == 0).all() and (few["pval"][1] == 0).all()


def test_errors_are_raised_at_sync_and_the_context_survives():
    G = 100
    S = np.random.default_rng(2).normal(size=(G, 2))
    ptr, rows = _csr([np.arange(10), np.arange(20) + 50])
    good = gficf_amd.gsea(S, ptr, rows, nsim=50, seed=SEED)
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = S.copy()
        bad[17, 1] = bad_value
        with pytest.raises(GficfError) as e:
            gficf_amd.gsea(bad, ptr, rows, nsim=50, seed=SEED)
        assert e.value.status == "GFICF_ERR_BAD_VALUE"
    for member in (G, -1):
        r2 = rows.copy()
        r2[3] = member
        with pytest.raises(GficfError) as e:
            gficf_amd.gsea(S, ptr, r2, nsim=50, seed=SEED)
        assert e.value.status == "GFICF_ERR_INVALID_ARG" and "outside" in str(e.value)
    r2 = rows.copy()
    r2[12] = r2[11]
    with pytest.raises(GficfError) as e:
        gficf_amd.gsea(S, ptr, r2, nsim=50, seed=SEED)
    assert e.value.status == "GFICF_ERR_INVALID_ARG" and "repeated" in str(e.value)
    with pytest.raises(GficfError) as e:
        gficf_amd.gsea(np.zeros((_gsea_lib.MAX_G + 1, 1)), ptr, rows, nsim=5)
    assert e.value.status == "GFICF_ERR_UNSUPPORTED"
    after = gficf_amd.gsea(S, ptr, rows, nsim=50, seed=SEED)
    for k in ("es", "nes", "pval"):
        assert _same_bits(after[k], good[k])


def test_largest_supported_gene_count():
    """G = 131 072: every word of the LDS mask, 16 words a thread."""
    G = _gsea_lib.MAX_G
    S = np.random.default_rng(3).normal(size=(G, 1))
    o = gs.order_desc(S[:, 0])
    sets = [o[:50], o[-50:], o[::1000], [o[G - 1]], np.arange(G - 1)]
    r = gficf_amd.gsea(S, *_csr(sets), nsim=2, seed=SEED, ret_null=True)
    want = np.array([[gs.es_of_set(gs.ranks(S[:, 0])[s], G)] for s in sets])
    assert _same_bits(r["es"], want) and r["es"][0, 0] == 1.0 and r["es"][1, 0] == -1.0
    assert _same_bits(r["null"], gs.null(G, SEED, r["sizes"], 2))


def test_fgsea_one_ranked_vector():
    import pandas as pd

    G = 400
    rng = np.random.default_rng(9)
    names = [f"g{i}" for i in range(G)]
    v = pd.Series(rng.normal(size=G), index=names)
    pw = {"a": ["g1", "g2", "g2", "nope", "g7"] + names[100:120], "small": ["g3", "zz"], "b": names[200:260]}
    df = gficf_amd.fgsea(pw, v, nsim=200, minSize=5, seed=SEED)
    assert list(df.columns) == ["pathway", "pval", "padj", "ES", "NES", "size"] and df["pathway"].tolist() == ["a", "b"]
    assert df["size"].tolist() == [23, 60]                   # matched, unique
    w = gs.gsea_np(v.to_numpy(), *_csr([[1, 2, 7] + list(range(100, 120)), [3], list(range(200, 260))]), nsim=200, min_size=5, seed=SEED)
    assert _same_bits(df["ES"], w["es"][[0, 2], 0]) and _same_bits(df["pval"], w["pval"][[0, 2], 0])
    assert _same_bits(df["padj"], gficf_amd.p_adjust_fdr(w["pval"][[0, 2], 0]))
    df2 = gficf_amd.fgsea(pw, v.to_numpy(), nsim=200, minSize=5, seed=SEED, names=names)
    assert df2.equals(df)


def test_run_gsea_end_to_end():
    import scipy.sparse as sp

    G, N, nsim = 600, 300, 1000
    rng = np.random.default_rng(11)
    planted = np.repeat(["A", "B", "C"], 100)
    lam = np.full((G, N), 0.3)
    for k in range(3):                                       # 60 genes up in each planted cluster
        lam[k * 60:(k + 1) * 60, k * 100:(k + 1) * 100] = 4.0
    M = sp.csc_matrix(rng.poisson(lam).astype(np.float64))
    data = gficf_amd.gficf(M, normalize=False, verbose=False)
    Gk = data["gficf"].shape[0]
    data["cluster.gene.rnk"], data["cluster.labels"] = gficf_amd.cluster_signatures(data["gficf"], planted)
    names = np.array([f"gene{g}" for g in data["genes"]])
    rnk = np.asarray(data["cluster.gene.rnk"])
    pw = {"top0": list(names[np.argsort(-rnk[:, 0], kind="stable")[:30]])}
    for i in range(40):
        pw[f"set{i}"] = list(names[rng.choice(Gk, int(rng.integers(15, 61)), replace=False)])
    pw["tiny"] = list(names[:5]) + ["not_a_gene"]           # below minSize once matched
    data = gficf_amd.runGSEA(data, nsim=nsim, pathways=pw, gene_names=names, verbose=False)
    g = data["gsea"]
    assert sorted(g) == ["es", "fdr", "nes", "pathways", "pval", "stat"] and g["pathways"] == pw
    row_of = {n: i for i, n in enumerate(names)}
    sets = [[row_of[m] for m in v if m in row_of] for v in pw.values()]
    ptr, rows = _csr(sets)
    w = gs.gsea_np(rnk, ptr, rows, nsim=nsim, min_size=15, seed=SEED)
    assert w["tested"].tolist() == [True] * 41 + [False]
    for k in ("es", "nes", "pval", "fdr"):
        assert list(g[k].index) == list(pw) and list(g[k].columns) == list(data["cluster.labels"]) == ["A", "B", "C"]
    r = {k: g[k].to_numpy() for k in ("es", "nes", "pval")}
    r.update(tested=w["tested"], size=w["size"])
    _check_against(r, w, nsim)
    fdr = np.zeros_like(w["pval"])
    for c in range(3):
        fdr[w["tested"], c] = gficf_amd.p_adjust_fdr(w["pval"][w["tested"], c])
    assert _same_bits(g["fdr"].to_numpy(), fdr)
    assert g["es"].loc["top0", "A"] == 1.0
    assert g["pval"].loc["top0", "A"] == 1 / (1 + w["nGeZero"][0, 0])
    assert g["fdr"].loc["top0", "A"] == g["fdr"]["A"].iloc[:41].min()
    assert g["stat"]["pathway"].tolist() == list(pw)[:41] and g["stat"]["size"].tolist() == [len(s) for s in sets[:41]]
    assert (g["es"].loc["tiny"] == 0).all() and (g["fdr"].loc["tiny"] == 0).all()
