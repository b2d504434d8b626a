"""GPU: the exact tail of the enrichment score (libgficf_gsea_exact.so) against the exact rational of
tests/helpers/gsea_exact_np.py.  Bar: relative error at most 4 G 2^-52 wherever the rational is at least 1e-290 (the contract of
include/gficf_gsea_exact.h), and the bits of the f64 port, which restates the library's order of operations; the same bits in
any batch and on every call.

Measured on one MI355X (error / bound, worst of each test): every attainable score at G <= 16: 0.030; G = 1200: 0.014;
m = 4095 among 4125: 0.0012; G = 131 072, m = 15: 0.0001."""
from fractions import Fraction
from math import comb

import numpy as np
import pytest

import gficf_amd
from gficf_amd import GficfError, _gsea_exact_lib
from tests.helpers import gsea_exact_np as gx

pytestmark = pytest.mark.gpu

SEED = 180582
TINY = Fraction(1, 10 ** 290)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _check(G, sizes, xs, got, port=True):
    """Every pair against the exact rational (and the port's bits); returns the worst error / bound."""
    worst = 0.0
    for m, x, g in zip(sizes, xs, got):
        want = gx.tail_exact(G, int(m), float(x))
        assert np.isfinite(g) and g >= 0, (G, m, x, g)
        if want >= TINY:
            r = float(abs(Fraction(float(g)) - want) / want) / gx.rel_bound(G)
            assert r <= 1.0, (G, m, x, g, float(want), r)
            worst = max(worst, r)
        else:
            assert Fraction(float(g)) <= want * (1 + Fraction(gx.rel_bound(G))), (G, m, x, g)
        if port:
            assert _same_bits(g, gx.tail_f64(G, int(m), float(x))), (G, m, x, g)
    return worst


def _set_scores(G, m, rng):
    """maxP and minP of the first m positions, the last m positions and a seeded random set."""
    sets = [np.arange(1, m + 1), np.arange(G - m + 1, G + 1), np.sort(rng.choice(G, m, replace=False)) + 1]
    return [v for S in sets for v in gx.max_min(S, G)]


@pytest.mark.parametrize("G", [2, 3, 7, 16])
def test_every_attainable_score(G):
    worst = 0.0
    for m in sorted({1, G // 2, G - 1}):
        pos, neg = gx.tail_enumerated(G, m)
        xs = np.array(list(pos) + list(neg))
        want = list(pos.values()) + list(neg.values())
        got = gficf_amd.gsea_tail(G, m, xs)
        assert got.shape == xs.shape
        for x, w, g in zip(xs, want, got):
            assert (g == 1.0) if x == 0 else (abs(Fraction(float(g)) - w) / w <= gx.rel_bound(G)), (G, m, x, g, w)
            assert g >= 1 / comb(G, m) * (1 - gx.rel_bound(G))          # a set counts itself
        worst = max(worst, _check(G, [m] * len(xs), xs, got))
    print(f"G={G}: worst error / bound {worst:.4f}")


def test_register_count_edges():
    """G = 1200; m on both sides of 64 R - 1 for R = 1, 2, 4, 8 and one size of R = 16.  The first and the last m positions have
    tails down to 1 / C(1200, 129) = 3.8e-177 (and below 1e-290 from m = 500 on): a form that cancelled would lose them."""
    G, rng = 1200, np.random.default_rng(SEED)
    sizes, xs = [], []
    for m in (1, 63, 64, 65, 127, 128, 129, 500, 513):
        s = _set_scores(G, m, rng)
        sizes += [m] * len(s)
        xs += s
    got = gficf_amd.gsea_tail(G, sizes, xs)
    assert len(got) == 54 and (got[np.asarray(xs) == 0] == 1.0).all()
    small = [g for m, x, g in zip(sizes, xs, got) if abs(x) == 1.0 and m == 129]
    assert small and all(3.8e-177 < g < 3.9e-177 for g in small)
    print(f"G=1200: worst error / bound {_check(G, sizes, xs, got):.4f}")


def test_largest_supported_size():
    m = _gsea_exact_lib.MAX_SIZE
    assert m >= 2048 and gx.reg_count(m) == 64
    G, rng = m + 30, np.random.default_rng(SEED + 1)         # thirty misses: every lane and register of R = 64 carries mass
    xs = [x for x in _set_scores(G, m, rng) if x != 0]
    got = gficf_amd.gsea_tail(G, m, xs)
    print(f"G={G} m={m}: worst error / bound {_check(G, [m] * len(xs), xs, got, port=False):.4f}")
    assert _same_bits(got[0], gx.tail_f64(G, m, xs[0]))


def test_limits():
    G = 131072
    # one hit: maxP >= top(1, j) holds for the j + 1 earliest positions, minP <= bottom(1, j) for the G - j latest
    js = np.array([0, 1, 1000, 65535, 65536, G - 2])
    got = gficf_amd.gsea_tail(G, 1, np.concatenate([gx.top(1, js, G, 1), gx.bottom(1, js, G, 1)]))
    want = np.concatenate([(js + 1) / G, (G - js) / G])
    assert np.abs(got / want - 1).max() <= gx.rel_bound(G)
    # fifteen hits among the first 3000 positions: a tail of 1e-25 on the positive side, a sweep of all G steps on the negative
    S = np.sort(np.random.default_rng(SEED + 2).choice(3000, 15, replace=False)) + 1
    xs = list(gx.max_min(S, G))
    got = gficf_amd.gsea_tail(G, 15, xs)
    assert got[0] < 1e-20 and got[1] > 0.5
    print(f"G={G} m=15: tails {got}, worst error / bound {_check(G, [15, 15], xs, got, port=False):.4f}")
    # m = G - 1
    xs = [x for x in _set_scores(300, 299, np.random.default_rng(3)) if x != 0]
    _check(300, [299] * len(xs), xs, gficf_amd.gsea_tail(300, 299, xs))
    # a size above the limit: NaN and no error, beside a pair that is computed
    over = _gsea_exact_lib.MAX_SIZE + 1
    got = gficf_amd.gsea_tail(over + 100, [over, 7], [0.5, 1.0])
    assert np.isnan(got[0]) and got[1] == pytest.approx(1 / comb(over + 100, 7), rel=gx.rel_bound(over + 100))
    with pytest.raises(GficfError) as e:
        gficf_amd.gsea_tail(G + 1, [5], [0.5])
    assert e.value.status == "GFICF_ERR_UNSUPPORTED" and "131072" in str(e.value)
    assert gficf_amd.gsea_tail(10, np.zeros(0, dtype=np.int32), np.zeros(0)).shape == (0,)


def test_underflow():
    got = gficf_amd.gsea_tail(4000, 200, [1.0, gx.max_min(np.arange(3801, 4001), 4000)[1]])
    assert np.isfinite(got).all() and (got >= 0).all() and (got < 1e-290).all()          # 1 / C(4000, 200) = 6e-344


@pytest.fixture(scope="module")
def mixed_pairs():
    G, rng = 700, np.random.default_rng(SEED + 3)
    sizes = np.concatenate([[1, 63, 64, 127, 128, 255, 256, 511, 512, 699], rng.integers(1, 700, 290)]).astype(np.int32)
    xs = np.array([gx.max_min(np.sort(rng.choice(G, int(m), replace=False)) + 1, G)[int(rng.integers(2))] for m in sizes])
    xs[5], xs[17] = 0.0, 1.0
    return G, sizes, xs


def test_determinism(mixed_pairs):
    G, sizes, xs = mixed_pairs
    single = np.array([gficf_amd.gsea_tail(G, [m], [x])[0] for m, x in zip(sizes, xs)])
    assert len(single) == 300 and (single > 0).all() and (single <= 1).all() and len({gx.reg_count(int(m)) for m in sizes}) == 5
    perm = np.random.default_rng(0).permutation(300)
    batch = gficf_amd.gsea_tail(G, sizes[perm], xs[perm])
    assert _same_bits(batch, single[perm])
    assert _same_bits(gficf_amd.gsea_tail(G, sizes[perm], xs[perm]), batch)
    some = perm[:12]
    _check(G, sizes[some], xs[some], single[some])


def test_device_resident_form_equals_the_host_form(mixed_pairs):
    import torch

    G, sizes, xs = mixed_pairs
    ops, dev = gficf_amd.HipOps(0), torch.device("cuda", 0)
    d_size, d_es = torch.from_numpy(sizes).to(dev), torch.from_numpy(xs).to(dev)
    tail = torch.full((300,), -1.0, dtype=torch.float64, device=dev)
    ws = torch.empty(ops.gsea_tail_workspace_bytes(G, 300), dtype=torch.uint8, device=dev)
    ops.gsea_tail(G, d_size, d_es, tail, ws)
    ops.gsea_tail_sync(ws)
    assert _same_bits(tail.cpu().numpy(), gficf_amd.gsea_tail(G, sizes, xs))
    with pytest.raises(GficfError, match="workspace too small"):
        ops.gsea_tail(G, d_size, d_es, tail, ws[:64])


def test_deferred_errors():
    good = gficf_amd.gsea_tail(50, [7, 7], [0.5, -0.5])
    for m, x, status, word in ((0, 0.5, "GFICF_ERR_INVALID_ARG", "size"), (50, 0.5, "GFICF_ERR_INVALID_ARG", "size"),
                               (-3, 0.5, "GFICF_ERR_INVALID_ARG", "size"), (7, np.nan, "GFICF_ERR_BAD_VALUE", "finite"),
                               (7, np.inf, "GFICF_ERR_BAD_VALUE", "finite"), (7, -1.5, "GFICF_ERR_BAD_VALUE", "finite"),
                               (7, np.nextafter(1.0, 2.0), "GFICF_ERR_BAD_VALUE", "finite")):
        with pytest.raises(GficfError) as e:
            gficf_amd.gsea_tail(50, [7, m, 7], [0.5, x, -0.5])
        assert e.value.status == status and word in str(e.value), (m, x)
        assert _same_bits(gficf_amd.gsea_tail(50, [7, 7], [0.5, -0.5]), good)          # the next call is clean
    _check(50, [7, 7], [0.5, -0.5], good)


# ------------------------------------------------------------------ the Python surface
@pytest.fixture(scope="module")
def planted():
    """2000 genes, two clusters (column 0 ranks the genes by row).  Pathways: the top 40 of column 0; its first and last gene
    (ES == 0 there: maxP = 1/2 = -minP); four spread sets; one gene alone, below min_size."""
    G, rng = 2000, np.random.default_rng(SEED + 4)
    stats = np.stack([-np.arange(G, dtype=np.float64), rng.normal(size=G)], axis=1)
    sets = [np.arange(40), np.array([0, G - 1])] + [rng.choice(G, int(k), replace=False) for k in (15, 40, 200, 700)] + [np.array([5])]
    ptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    return G, stats, ptr, np.concatenate(sets).astype(np.int32)


def test_gsea_exact_outputs(planted):
    G, stats, ptr, rows = planted
    nsim = 200
    a = gficf_amd.gsea(stats, ptr, rows, nsim=nsim, min_size=2, seed=SEED, ret_null=True)
    b = gficf_amd.gsea(stats, ptr, rows, nsim=nsim, min_size=2, seed=SEED, ret_null=True, exact=True)
    assert set(b) == set(a) | {"ptail", "pval_exact"} and set(gficf_amd.gsea(stats, ptr, rows, nsim=nsim, min_size=2, seed=SEED)) == set(a) - {"sizes", "null"}
    for k in ("es", "nes", "pval", "null"):
        assert _same_bits(a[k], b[k]), k
    assert "null" not in gficf_amd.gsea(stats, ptr, rows, nsim=nsim, min_size=2, seed=SEED, exact=True)
    es, ptail, pe = b["es"], b["ptail"], b["pval_exact"]
    assert ptail.shape == pe.shape == es.shape == (7, 2) and list(b["tested"]) == [True] * 6 + [False]
    assert (ptail[6] == 0).all() and (pe[6] == 0).all() and es[1, 0] == 0.0 and ptail[1, 0] == 1.0 and pe[1, 0] == 1.0
    t = np.flatnonzero(b["tested"])
    assert _same_bits(ptail[t], gficf_amd.gsea_tail(G, b["size"][t][:, None], es[t]))
    d = np.searchsorted(b["sizes"], b["size"][t])
    n_ge, n_le = (b["null"] >= 0).sum(axis=1)[d], (b["null"] <= 0).sum(axis=1)[d]
    for r, p in enumerate(t):
        for c in range(2):
            n0 = n_ge[r] if es[p, c] > 0 else n_le[r]
            want = 1.0 if es[p, c] == 0 else min(1.0, ptail[p, c] * np.float64(nsim + 1) / np.float64(n0 + 1))
            assert _same_bits(pe[p, c], want), (p, c)
    # the planted set: the simple estimator is at its floor for this size, 1 / (1 + nGeZero) (1 / (nsim + 1) if no null value is negative)
    assert es[0, 0] == 1.0 and 1 / (nsim + 1) <= b["pval"][0, 0] == 1 / (1 + n_ge[0]) and pe[0, 0] < 1e-30
    assert ptail[0, 0] == pytest.approx(1 / comb(G, 40), rel=gx.rel_bound(G))
    assert ((pe[t] > 0) & (pe[t] <= 1)).all()


def test_a_set_above_the_size_limit_keeps_the_simple_pvalue():
    G, over = 4300, _gsea_exact_lib.MAX_SIZE + 1
    stats = -np.arange(G, dtype=np.float64)
    ptr, rows = np.array([0, over, over + 30], dtype=np.int64), np.concatenate([np.arange(over), np.arange(30)]).astype(np.int32)
    with pytest.warns(UserWarning, match=f"GFICF_GSEA_EXACT_MAX_SIZE = {over - 1}"):
        r = gficf_amd.gsea(stats, ptr, rows, nsim=20, seed=SEED, exact=True)
    assert np.isnan(r["ptail"][0, 0]) and 1 / 21 <= r["pval_exact"][0, 0] == r["pval"][0, 0] <= 1
    assert r["ptail"][1, 0] == pytest.approx(1 / comb(G, 30), rel=gx.rel_bound(G)) and r["pval_exact"][1, 0] < 1e-60


def test_run_gsea_and_fgsea_exact(planted):
    import pandas as pd

    G, stats, ptr, rows = planted
    names = np.array([f"g{i}" for i in range(G)])
    sets = {f"p{k}": list(names[rows[ptr[k]:ptr[k + 1]]]) for k in range(len(ptr) - 1)}
    data = {"cluster.gene.rnk": stats, "gene_names": names, "cluster.labels": ["a", "b"]}
    old = gficf_amd.runGSEA(dict(data), nsim=200, pathways=sets, minSize=2, verbose=False, seed=SEED)["gsea"]
    new = gficf_amd.runGSEA(dict(data), nsim=200, pathways=sets, minSize=2, verbose=False, seed=SEED, exact=True)["gsea"]
    assert set(new) == set(old) | {"ptail", "pval_exact", "fdr_exact"} and set(old) == {"pathways", "es", "nes", "pval", "fdr", "stat"}
    for k in ("es", "nes", "pval", "fdr"):
        assert _same_bits(old[k].to_numpy(), new[k].to_numpy()) and list(new[k].index) == list(sets) and list(new[k].columns) == ["a", "b"], k
    assert new["stat"].equals(old["stat"])
    pe, fe = new["pval_exact"].to_numpy(), new["fdr_exact"].to_numpy()
    for c in range(2):
        assert _same_bits(fe[:6, c], gficf_amd.p_adjust_fdr(pe[:6, c]))          # BH over the six tested pathways
    assert (fe[6] == 0).all() and (pe[6] == 0).all() and (new["ptail"].to_numpy()[6] == 0).all()
    assert pe[0, 0] < 1e-30 and fe[0, 0] < 1e-29 and 1 / 201 <= old["pval"].iloc[0, 0] <= old["pval"].to_numpy()[:6].min()
    f0 = gficf_amd.fgsea(sets, pd.Series(stats[:, 0], index=names), nsim=200, minSize=2, seed=SEED)
    f1 = gficf_amd.fgsea(sets, pd.Series(stats[:, 0], index=names), nsim=200, minSize=2, seed=SEED, exact=True)
    assert list(f0.columns) == ["pathway", "pval", "padj", "ES", "NES", "size"] and list(f1.columns) == list(f0.columns) + ["pval_simple"]
    assert _same_bits(f1["pval_simple"], f0["pval"]) and _same_bits(f1["pval"], pe[:6, 0]) and _same_bits(f1["padj"], fe[:6, 0])
    assert _same_bits(f1["ES"], f0["ES"]) and _same_bits(f1["NES"], f0["NES"])
