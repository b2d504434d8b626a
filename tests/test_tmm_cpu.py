"""No GPU: the NumPy oracle of libgficf_tmm.so (tests/helpers/tmm_np.py, the yardstick of tests/test_tmm_gpu.py) against
answers derived by hand and against edgeR's literal ranks, the header against its loader and the Makefile, and the argument
handling of the Python mirror."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import gficf_amd
from gficf_amd import synth
from tests.helpers import tmm_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_loader_name_the_same_entries():
    from gficf_amd import _tmm_lib

    text = open(os.path.join(ROOT, "include", "gficf_tmm.h")).read()
    body = text[text.index("extern \"C\""):]
    declared = re.findall(r"\b(gficf_tmm_\w+)\s*\(([^;]*)\)\s*;", body)
    assert set(n for n, _ in declared) == set(_tmm_lib.SIGNATURES) and len(declared) == 7
    for name, args in declared:
        n = 0 if args.strip() == "void" else args.count(",") + 1
        assert n == len(_tmm_lib.SIGNATURES[name][1]), name
    assert "#define GFICF_TMM_ABI_VERSION 1" in text and _tmm_lib.ABI_VERSION == 1
    assert re.search(rf"#define\s+GFICF_TMM_LDS_N\s+{_tmm_lib.LDS_N}\b", text) and 2 * 8 * _tmm_lib.LDS_N <= 160 * 1024
    core = open(os.path.join(ROOT, "include", "gficf_hip.h")).read()
    assert re.search(r"#define\s+GFICF_HIP_ABI_VERSION\s+7\b", core)


def test_makefile_builds_the_library_with_the_others():
    csrc = os.path.join(ROOT, "gficf_amd", "csrc")
    build = subprocess.run(["make", "-n", "-B", "-C", csrc, "all"], capture_output=True, text=True, check=True).stdout.splitlines()
    link = [ln for ln in build if " -o ../libgficf_tmm.so " in ln]
    assert len(link) == 1 and re.search(r"hipcc --offload-arch=gfx950 -shared -fPIC -o \.\./libgficf_tmm\.so tmm\.o -L\.\. -lgficf_hip\b", link[0])
    comp = [ln for ln in build if ln.endswith(" -o tmm.o")]
    assert len(comp) == 1 and "-ffp-contract=off" in comp[0] and "--offload-arch=gfx950" in comp[0] and "fast-math" not in comp[0]
    assert build.index(link[0]) > max(i for i, ln in enumerate(build) if " -o ../libgficf_hip.so " in ln or ln.endswith(" -o tmm.o"))
    clean = subprocess.run(["make", "-n", "-C", csrc, "clean"], capture_output=True, text=True, check=True).stdout
    assert re.search(r"^rm -f .*\btmm\.o\b.* \.\./libgficf_tmm\.so\b", clean, re.M)


def test_loader(monkeypatch):
    from gficf_amd import _tmm_lib

    L = _tmm_lib.load()
    assert isinstance(L, ctypes.CDLL) and _tmm_lib.load() is L and L.gficf_tmm_abi_version() == _tmm_lib.ABI_VERSION
    for sym, (res, args) in _tmm_lib.SIGNATURES.items():
        fn = getattr(L, sym)
        assert fn.restype is res and list(fn.argtypes) == list(args), sym
    assert os.path.basename(_tmm_lib.LIB_PATH) == "libgficf_tmm.so"
    small = L.gficf_tmm_workspace_bytes(23000, 54000, 0, 0)
    assert 12 * 23000 + 4 * 54000 < small < 12 * 23000 + 4 * 54000 + 4096 and L.gficf_tmm_workspace_bytes(23000, 54000, 3, 30000) >= small + 16 * 30000 - 1024
    assert L.gficf_tmm_workspace_bytes(0, 10, 0, 0) == 0 and L.gficf_tmm_workspace_bytes(10, 10, -1, 0) == 0
    monkeypatch.setattr(_tmm_lib, "LIB_PATH", os.path.join(os.path.dirname(_tmm_lib.LIB_PATH), "libgficf_tmm_missing.so"))
    with pytest.raises(ImportError, match="not found: build it with"):
        _tmm_lib.load()


# ------------------------------------------------------------------ the oracle against what defines it
def test_quantile_is_numpys_linear_quantile_over_the_rows_that_hold_a_count():
    X = tmm_np.gamma_poisson(300, 40, seed=1)
    X[::7] = 0                                                            # all-zero rows: G' < G
    lib, sq, f75, ostat, Gp = tmm_np.col_stats(X)
    assert Gp == int((X > 0).any(axis=1).sum()) < 300
    want = np.quantile(X[(X > 0).any(axis=1)], .75, axis=0) / X.sum(axis=0)
    np.testing.assert_allclose(f75, want, rtol=1e-14)
    assert (ostat[0] <= ostat[1]).all() and np.array_equal(lib, X.sum(axis=0))


def test_average_rank_is_scipys_rankdata():
    from scipy.stats import rankdata

    rng = np.random.default_rng(0)
    for n in (1, 2, 7, 100):
        v = rng.integers(1, 6, n).astype(np.float64)
        assert np.array_equal(tmm_np.avg_rank(v), rankdata(v))


def test_the_two_rank_modes_are_bit_equal_without_ties():
    rng = np.random.default_rng(4)
    X = rng.lognormal(0.0, 1.0, (800, 40)) * (rng.random((800, 40)) < .4)
    a = tmm_np.calc_norm_factors(X, keys="canonical")
    b = tmm_np.calc_norm_factors(X, keys="literal")
    assert a["refColumn"] == b["refColumn"] and np.array_equal(a["kept"], b["kept"]) and np.array_equal(a["n"], b["n"])
    assert np.array_equal(a["norm.factors"], b["norm.factors"]) and (a["kept"] < a["n"]).any()
    for c in range(40):                                                   # the kept sets themselves
        ka = tmm_np.cell_factor(X[:, c], X[:, a["refColumn"]], a["lib.size"][c], a["lib.size"][a["refColumn"]], keys="canonical")[3]
        kb = tmm_np.cell_factor(X[:, c], X[:, a["refColumn"]], a["lib.size"][c], a["lib.size"][a["refColumn"]], keys="literal")[3]
        assert np.array_equal(ka, kb)


def test_the_rank_modes_differ_on_integer_counts():
    """Recorded, not bounded: on synth.counts_csc(2000, 300, 0.07) the literal ranks (ties made and broken by
    the rounding of log2 and the divisions) change the kept set of 5 of the 300 cells, and a factor by up to 8.8 %."""
    colptr, rowidx, x = synth.counts_csc(2000, 300, 0.07)
    X = sp.csc_matrix((x, rowidx, colptr), shape=(2000, 300)).toarray()
    a = tmm_np.calc_norm_factors(X, keys="canonical")
    b = tmm_np.calc_norm_factors(X, keys="literal")
    assert a["refColumn"] == b["refColumn"] and np.array_equal(a["n"], b["n"])
    ref, lib = a["refColumn"], a["lib.size"]
    cells = sum(not np.array_equal(tmm_np.cell_factor(X[:, c], X[:, ref], lib[c], lib[ref], keys="canonical")[3],
                                   tmm_np.cell_factor(X[:, c], X[:, ref], lib[c], lib[ref], keys="literal")[3]) for c in range(300))
    worst = float(np.abs(b["norm.factors"] / a["norm.factors"] - 1).max())
    print(f"literal vs canonical ranks: kept set differs in {cells} of 300 cells, largest factor deviation {worst:.3g}")
    assert cells > 0 and worst > 0


def test_reference_columns_of_the_gpu_inputs_are_chosen_with_room():
    colptr, rowidx, x = synth.counts_csc(2000, 300, 0.07)
    X = sp.csc_matrix((x, rowidx, colptr), shape=(2000, 300)).toarray()
    _, sq, f75, _, _ = tmm_np.col_stats(X)
    assert np.median(f75) < 1e-20 and tmm_np.choose_ref(f75, sq)[1] > 1e-9          # the sq branch
    _, sq, f75, _, _ = tmm_np.col_stats(tmm_np.gamma_poisson())
    assert np.median(f75) > 1e-20 and tmm_np.choose_ref(f75, sq)[1] > 1e-9          # the f75 branch
    X, _ = tmm_np.edge_matrix()
    _, sq, f75, _, _ = tmm_np.col_stats(X)
    assert np.median(f75) < 1e-20 and tmm_np.choose_ref(f75, sq)[0] in (0, len(tmm_np.EDGE_N) + 1)


# ------------------------------------------------------------------ derived answers, no oracle in the loop
def test_derived_answers_hold_for_the_oracle():
    X = tmm_np.multiples_matrix()
    res = tmm_np.calc_norm_factors(X, refColumn=0)
    tmm_np.check_multiples(X, res, tmm_np.cpm(X, res["lib.size"], res["norm.factors"]))
    X, changed = tmm_np.boosted_matrix()
    res = tmm_np.calc_norm_factors(X, refColumn=0)
    tmm_np.check_boosted(X, changed, res, tmm_np.cpm(X, res["lib.size"], res["norm.factors"]))


def test_trim_products_are_taken_in_f64_as_written():
    # n = 10: floor(10 * 0.3) = floor(3.0000000000000004) = 3, so ranks 4 .. 7 survive the logR trim
    rng = np.random.default_rng(2)
    obs, ref = rng.lognormal(0, 1, 10), rng.lognormal(0, 1, 10)
    _, n, kept, keep = tmm_np.cell_factor(obs, ref, obs.sum(), ref.sum(), sumTrim=0.0)
    assert n == 10 and kept == 4 and np.array_equal(np.sort(tmm_np.avg_rank(obs / ref)[keep]), [4, 5, 6, 7])


# ------------------------------------------------------------------ the mirror's argument handling
def test_argument_errors():
    M = sp.csc_matrix(np.ones((4, 6)))
    with pytest.raises(ValueError, match="logratioTrim"):
        gficf_amd.calcNormFactors(M, logratioTrim=.5)
    with pytest.raises(ValueError, match="sumTrim"):
        gficf_amd.calcNormFactors(M, sumTrim=-1)
    with pytest.raises(ValueError, match="refColumn"):
        gficf_amd.calcNormFactors(M, refColumn=6)
    with pytest.raises(ValueError, match="one value per cell"):
        gficf_amd.cpm(M, lib_size=np.ones(5))
    with pytest.raises(ValueError, match='True, False or "tmm"'):
        gficf_amd.gficf(M, normalize="edgeR", verbose=False)
    with pytest.raises(ValueError, match='a matrix, None or "tmm"'):
        gficf_amd.findClusterMarkers({"community": np.zeros(6), "rawCounts": M}, hvg=False, cpms="cpm")
    import inspect

    sig = inspect.signature(gficf_amd.calcNormFactors).parameters
    assert list(sig)[:5] == ["M", "refColumn", "logratioTrim", "sumTrim", "doWeighting"]
    assert (sig["logratioTrim"].default, sig["sumTrim"].default, sig["doWeighting"].default) == (.3, .05, True)
    sig = inspect.signature(gficf_amd.normCounts).parameters
    assert (sig["doc_proportion_max"].default, sig["doc_proportion_min"].default, sig["normalizeCounts"].default) == (1, .01, False)
