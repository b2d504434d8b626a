"""No GPU: the NumPy oracle of libgficf_gsva.so (tests/helpers/gsva_np.py, the yardstick of tests/test_gsva_gpu.py) against
what defines it, the header against its loader and the Makefile, and the argument handling of the Python mirror."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
from scipy import stats

import gficf_amd
from gficf_amd import _gsva_lib
from tests.helpers import gsva_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_loader_name_the_same_entries():
    text = open(os.path.join(ROOT, "include", "gficf_gsva.h")).read()
    body = text[text.index("extern \"C\""):]
    declared = re.findall(r"\b(gficf_gsva_\w+)\s*\(([^;]*)\)\s*;", body)
    assert set(n for n, _ in declared) == set(_gsva_lib.SIGNATURES) and len(declared) == 7
    for name, args in declared:
        n = 0 if args.strip() == "void" else args.count(",") + 1
        assert n == len(_gsva_lib.SIGNATURES[name][1]), name
    assert "#define GFICF_GSVA_ABI_VERSION 1" in text and _gsva_lib.ABI_VERSION == 1
    for name in ("MAX_G", "MAX_CELL_NZ", "TILE", "JSPLIT"):
        assert re.search(rf"#define\s+GFICF_GSVA_{name}\s+{getattr(_gsva_lib, name)}\b", text), name
    core = open(os.path.join(ROOT, "include", "gficf_hip.h")).read()
    assert re.search(r"#define\s+GFICF_HIP_ABI_VERSION\s+7\b", core)


def test_makefile_builds_the_library_with_the_others():
    csrc = os.path.join(ROOT, "gficf_amd", "csrc")
    build = subprocess.run(["make", "-n", "-B", "-C", csrc, "all"], capture_output=True, text=True, check=True).stdout.splitlines()
    link = [ln for ln in build if " -o ../libgficf_gsva.so " in ln]
    assert len(link) == 1 and re.search(r"hipcc --offload-arch=gfx950 -shared -fPIC -o \.\./libgficf_gsva\.so gsva\.o -L\.\. -lgficf_hip\b", link[0])
    comp = [ln for ln in build if ln.endswith(" -o gsva.o")]
    assert len(comp) == 1 and "-ffp-contract=off" in comp[0] and "--offload-arch=gfx950" in comp[0]
    assert build.index(link[0]) > max(i for i, ln in enumerate(build) if " -o ../libgficf_hip.so " in ln or ln.endswith(" -o gsva.o"))
    clean = subprocess.run(["make", "-n", "-C", csrc, "clean"], capture_output=True, text=True, check=True).stdout
    assert re.search(r"^rm -f .*\bgsva\.o\b.* \.\./libgficf_gsva\.so\b", clean, re.M)


def test_loader(monkeypatch):
    L = _gsva_lib.load()
    assert isinstance(L, ctypes.CDLL) and _gsva_lib.load() is L and L.gficf_gsva_abi_version() == _gsva_lib.ABI_VERSION
    for sym, (res, args) in _gsva_lib.SIGNATURES.items():
        fn = getattr(L, sym)
        assert fn.restype is res and list(fn.argtypes) == list(args), sym
    assert os.path.basename(_gsva_lib.LIB_PATH) == "libgficf_gsva.so"
    assert L.gficf_gsva_workspace_bytes(2000, 600, 4, 50) > 44 * 2000 * 4 and L.gficf_gsva_workspace_bytes(_gsva_lib.MAX_G + 1, 600, 4, 50) == 0
    monkeypatch.setattr(_gsva_lib, "LIB_PATH", os.path.join(os.path.dirname(_gsva_lib.LIB_PATH), "libgficf_gsva_missing.so"))
    with pytest.raises(ImportError, match="not found: build it with"):
        _gsva_lib.load()


# ------------------------------------------------------------------ the oracle against what defines it
@pytest.mark.parametrize("n,nz", [(2, 1), (3, 3), (17, 5), (40, 0), (40, 39), (300, 120)])
def test_sparse_density_equals_the_dense_sum(n, nz):
    rng = np.random.default_rng(1000 * n + nz)
    x = np.zeros(n)
    x[rng.permutation(n)[:nz]] = rng.lognormal(0.0, 1.0, nz) * rng.choice([-1.0, 1.0], nz)
    if nz == 0:
        assert not gsva_np.gene_filter(x[None, :])[1][0]                 # a constant gene is dropped, nothing to compare
        return
    sd, kept = gsva_np.gene_filter(x[None, :])
    assert kept[0] and abs(sd[0] - np.std(x, ddof=1)) <= 1e-14 * sd[0]
    dense = gsva_np.density_dense(x, sd[0])
    d_nz, d0 = gsva_np.density_sparse(x[x != 0], n, sd[0])
    assert np.isfinite(dense).all()
    np.testing.assert_allclose(d_nz, dense[x != 0], rtol=1e-12, atol=1e-13)
    if nz < n:
        np.testing.assert_allclose(np.full(n - nz, d0), dense[x == 0], rtol=1e-12, atol=1e-13)
    L = 1.0 / (1.0 + np.exp(-dense))
    assert (L >= 0.5 / n - 1e-15).all() and (L <= 1 - 0.5 / n + 1e-15).all()


def test_phi_is_the_normal_cdf():
    v = np.array([-12.0, -3.0, -0.5, 0.0, 0.5, 3.0, 12.0])
    np.testing.assert_allclose(gsva_np.phi(v), stats.norm.cdf(v), rtol=1e-13, atol=0)


@pytest.mark.parametrize("Gc", [2, 7, 40, 41, 300])
def test_closed_form_equals_the_sequential_walk(Gc):
    rng = np.random.default_rng(Gc)
    worst = 0.0
    for m in sorted({1, 2, Gc // 3 + 1, Gc - 1}):
        if not 1 <= m <= Gc - 1:
            continue
        for _ in range(20):
            S = np.sort(rng.permutation(Gc)[:m] + 1)
            a, b = gsva_np.es_closed(S, Gc), gsva_np.es_walk(S, Gc)
            if np.isnan(a) or np.isnan(b):
                assert np.isnan(a) and np.isnan(b) and m == 1 and Gc % 2 == 0 and S[0] == Gc // 2 + 1
                continue
            worst = max(worst, abs(a - b))
    assert worst < 1e-13, worst                                          # the rounding of Gc sequential additions of steps <= 1


def test_zero_weight_is_nan_only_on_the_middle_gene():
    for Gc in (6, 7, 40):
        got = [np.isnan(gsva_np.es_closed([S], Gc)) for S in range(1, Gc + 1)]
        assert got == [Gc % 2 == 0 and S == Gc // 2 + 1 for S in range(1, Gc + 1)]


@pytest.mark.parametrize("Gc,m", [(10, 3), (41, 7), (300, 150)])
def test_top_set_is_positive_and_the_reversed_order_negates_it(Gc, m):
    top = np.arange(1, m + 1)
    es = gsva_np.es_closed(top, Gc)
    assert es > 0 and es == gsva_np.es_closed(top, Gc) and abs(es - 1.0) < 1e-15      # every step up comes first
    mirrored = Gc + 1 - top                                              # the same set under the complement ordering
    assert gsva_np.es_closed(mirrored, Gc) == -es
    assert abs(gsva_np.es_walk(mirrored, Gc) + gsva_np.es_walk(top, Gc)) < 1e-13


def test_positions_break_ties_by_row():
    assert list(gsva_np.positions([1.0, 3.0, 1.0, -0.0, 0.0, 3.0])) == [3, 1, 4, 5, 6, 2]


def _scores_matrix(seed, P=12, n1=9, n2=14, shift=0.0):
    rng = np.random.default_rng(seed)
    Y = rng.normal(0.0, 0.3, (P, n1 + n2))
    Y[:, :n1] += shift
    return Y, np.arange(n1 + n2) < n1


def test_limma_sign_and_the_infinite_prior_limit():
    # rows that differ only by a shift of the cluster's cells have one residual variance: the variance of log s^2 is not
    # positive, df0 = inf, the posterior variance is the common s^2 and the moderated t is Student's pooled-variance t of
    # scipy.stats.ttest_ind; its degrees of freedom are the pooled P' * (N - 2), which limma caps df + df0 with
    y, inc = _scores_matrix(1, P=1)
    shifts = np.linspace(-0.5, 0.5, 12)
    Y = y + shifts[:, None] * inc[None, :]
    r = gsva_np.limma_cluster_vs_rest(Y, inc)
    assert np.isinf(r["df0"])
    ref = [stats.ttest_ind(row[~inc], row[inc]) for row in Y]
    t = np.array([x.statistic for x in ref])
    np.testing.assert_allclose(r["logFC"], Y[:, ~inc].mean(axis=1) - Y[:, inc].mean(axis=1), rtol=1e-12, atol=1e-15)   # mean(other) - mean(cluster)
    assert (np.diff(r["logFC"]) < 0).all()                              # the more the cluster is lifted, the lower logFC
    np.testing.assert_allclose(r["t"], t, rtol=1e-10)
    np.testing.assert_allclose(r["P.Value"], 2 * stats.t.sf(np.abs(t), 12 * (Y.shape[1] - 2)), rtol=1e-9)
    assert (r["P.Value"] <= np.array([x.pvalue for x in ref]) * (1 + 1e-12)).all()     # Student's own has N - 2 degrees of freedom
    flipped = gsva_np.limma_cluster_vs_rest(Y, inc, cluster_minus_other=True)
    assert np.array_equal(flipped["logFC"], -r["logFC"]) and np.array_equal(flipped["t"], -r["t"]) and np.array_equal(flipped["P.Value"], r["P.Value"])


def test_limma_with_one_row_is_the_two_sample_t_test():
    # a single row has no prior to borrow from (df0 = 0): the moderated t is Student's pooled-variance t
    Y, inc = _scores_matrix(7, P=1, shift=0.4)
    r = gsva_np.limma_cluster_vs_rest(Y, inc)
    ref = stats.ttest_ind(Y[0, ~inc], Y[0, inc])
    assert r["df0"] == 0.0 and r["logFC"][0] < 0
    np.testing.assert_allclose([r["t"][0], r["P.Value"][0]], [ref.statistic, ref.pvalue], rtol=1e-10)


def test_limma_shrinks_towards_the_prior_when_variances_differ():
    rng = np.random.default_rng(5)
    Y, inc = _scores_matrix(11, P=30)
    Y *= rng.lognormal(0.0, 1.0, 30)[:, None]
    r = gsva_np.limma_cluster_vs_rest(Y, inc)
    assert 0 < r["df0"] < np.inf
    plain = np.array([stats.ttest_ind(y[~inc], y[inc]).statistic for y in Y])
    assert np.array_equal(np.sign(r["t"]), np.sign(plain)) and not np.allclose(r["t"], plain)
    assert np.all(np.diff(r["adj.P.Val"][np.argsort(r["P.Value"])]) >= 0) and (r["adj.P.Val"] >= r["P.Value"]).all()
    np.testing.assert_allclose(r["adj.P.Val"], gficf_amd.p_adjust_fdr(r["P.Value"]), rtol=0, atol=0)
    assert abs(special_trigamma(gsva_np.trigamma_inverse(0.37)) - 0.37) < 1e-12


def special_trigamma(y):
    from scipy.special import polygamma

    return float(polygamma(1, y))


def test_mirror_finish_equals_the_oracle_limma_on_host_sums():
    # gsva_de_pathways reads sums; given sums taken in NumPy it must reproduce the least-squares oracle
    rng = np.random.default_rng(3)
    cluster = rng.integers(0, 3, 60)
    es = rng.normal(0, 0.3, (9, 60)) + 0.2 * (cluster == 1)
    es[4] = 0.0                                                          # an all-zero row is dropped
    S = np.stack([es[:, cluster == c].sum(axis=1) for c in range(3)], axis=1)
    Q = np.stack([(es[:, cluster == c] ** 2).sum(axis=1) for c in range(3)], axis=1)
    for flip in (False, True):
        got = gficf_amd.gsva_de_pathways({"sum": S, "sumsq": Q}, cluster, cluster_minus_other=flip)
        want = gsva_np.de_pathways(es, cluster, 3, flip)
        assert list(got.columns) == ["logFC", "AveExpr", "t", "P.Value", "adj.P.Val", "pathway", "cluster"] and len(got) == 3 * 8
        assert np.array_equal(got["pathway"].to_numpy(), want["pathway"]) and np.array_equal(got["cluster"].to_numpy(), want["cluster"])
        for k in ("logFC", "AveExpr", "t", "P.Value", "adj.P.Val"):
            np.testing.assert_allclose(got[k].to_numpy(), want[k], rtol=1e-10, atol=0, err_msg=k)


# ------------------------------------------------------------------ the mirror's argument handling
def test_run_gsva_argument_errors(tmp_path):
    import scipy.sparse as sp

    f = tmp_path / "sets.gmt"
    f.write_text("A\tx\tg1\tg2\n")
    M = sp.csc_matrix(np.ones((4, 6)))
    with pytest.raises(ValueError, match="Please run gficf function first"):
        gficf_amd.runGSVA({}, str(f))
    with pytest.raises(ValueError, match="Please run clustcell function first"):
        gficf_amd.runGSVA({"gficf": M}, str(f))
    data = {"gficf": M, "cluster": np.array(["1", "1", "1", "2", "2", "2"])}
    with pytest.raises(ValueError, match="gmt_file or pathways"):
        gficf_amd.runGSVA(data, verbose=False)
    with pytest.raises(NotImplementedError, match="gene_map"):
        gficf_amd.runGSVA(data, str(f), convertToEns=True, verbose=False, gene_names=["g1", "g2", "g3", "g4"])
    with pytest.raises(ValueError, match="gene_names"):
        gficf_amd.runGSVA(data, str(f), verbose=False)
    with pytest.raises(ValueError, match="gene_names"):
        gficf_amd.runGSVA(data, str(f), verbose=False, gene_names=["g1", "g2"])
    with pytest.raises(ValueError, match="one label per cell"):
        gficf_amd.runGSVA({"gficf": M, "cluster": np.array(["1", "2"])}, str(f), verbose=False, gene_names=["g1", "g2", "g3", "g4"])


def test_gsva_argument_errors():
    import scipy.sparse as sp

    M = sp.csr_matrix(np.ones((4, 6)))
    cl = np.zeros(6, dtype=np.int32)
    with pytest.raises(ValueError, match="one integer id per cell"):
        gficf_amd.gsva(M, np.zeros(5, dtype=np.int32), [0, 2], [0, 1])
    with pytest.raises(ValueError, match="one integer id per cell"):
        gficf_amd.gsva(M, np.zeros(6), [0, 2], [0, 1])
    with pytest.raises(ValueError, match="ptr must hold"):
        gficf_amd.gsva(M, cl, [0, 3], [0, 1])
    with pytest.raises(ValueError, match="NaN"):
        gficf_amd.gsva(M, cl, [0, 2], [0, 1], min_size=float("nan"))
    with pytest.raises(ValueError, match="n_clusters"):
        gficf_amd.gsva(M, cl, [0, 2], [0, 1], n_clusters=0)
    with pytest.raises(ValueError, match="d0 and kept must be G x C"):
        gficf_amd.gsva_scores(np.zeros(24), np.zeros((4, 2)), np.ones((4, 1)), M, cl, [0, 2], [0, 1])
    with pytest.raises(ValueError, match="what gsva"):
        gficf_amd.gsva_de_pathways({"es": np.zeros((2, 6))}, cl)


def test_run_gsea_names_run_gsva():
    with pytest.raises(NotImplementedError, match="runGSVA"):
        gficf_amd.runGSEA({"cluster.gene.rnk": np.ones((4, 2))}, "unused.gmt", method="GSVA", verbose=False)
    import inspect

    sig = inspect.signature(gficf_amd.runGSVA)
    assert list(sig.parameters)[:10] == ["data", "gmt_file", "minSize", "maxSize", "pathways", "gene_names", "convertToEns", "gene_map", "nt", "verbose"]
    assert sig.parameters["minSize"].default == 15 and sig.parameters["cluster_minus_other"].default is False
    assert inspect.signature(gficf_amd.gsva_de_pathways).parameters["cluster_minus_other"].default is False
