"""No GPU: the yardsticks of libgficf_gsea_exact.so (tests/helpers/gsea_exact_np.py, which tests/test_gsea_exact_gpu.py measures
the library against) checked against what defines them: the exact count against the enumeration of every subset, the f64 port
against the exact count, both against the library's own sampler; the header against its loader and the Makefile; the argument
handling of the new keywords."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess
from fractions import Fraction
from math import comb

import numpy as np
import pytest

import gficf_amd
from tests.helpers import gsea_exact_np as gx
from tests.helpers import gsea_np as gs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENUM = [(2, 1), (3, 1), (7, 3), (9, 1), (10, 4), (12, 6), (13, 12), (14, 5)]


def _ratio(got, want, G):
    """The relative error of ``got`` against the Fraction ``want`` in units of the contract's bound 4 G 2^-52."""
    return float(abs(Fraction(got) - want) / want) / gx.rel_bound(G)


@pytest.mark.parametrize("G,m", ENUM)
def test_exact_count_equals_enumeration(G, m):
    pos, neg = gx.tail_enumerated(G, m)
    assert len(pos) >= 1 and len(neg) >= 1 and max(pos.values()) == 1 and max(neg.values()) == 1
    worst = 0.0
    for x, share in list(pos.items()) + list(neg.items()):
        assert gx.tail_exact(G, m, x) == share, (G, m, x)
        got = gx.tail_f64(G, m, x)
        if x == 0:
            assert got == 1.0
        else:
            worst = max(worst, _ratio(got, share, G))
    print(f"G={G} m={m}: {len(pos)} + {len(neg)} scores, port error / bound {worst:.4f}")
    assert worst <= 1.0


def test_the_sign_is_not_a_fair_coin():
    """Mathematically tied sets split by the last bit of the f64 expressions: 478 positive, 400 negative at G = 12, m = 6."""
    from itertools import combinations

    es = np.array([gs.es_positions(S, 12) for S in combinations(range(1, 13), 6)])
    assert ((es > 0).sum(), (es < 0).sum(), (es == 0).sum()) == (478, 400, 46)


@pytest.mark.parametrize("m", [1, 63, 64, 65, 129, 500])
def test_port_accuracy(m):
    G = 1200
    S = np.sort(np.random.default_rng(m).choice(G, m, replace=False)) + 1
    xs = [gx.max_min(S, G)[0], gx.max_min(S, G)[1], 1.0, gx.max_min(np.arange(G - m + 1, G + 1), G)[1]]
    for x in xs:
        want, got = gx.tail_exact(G, m, x), gx.tail_f64(G, m, x)
        assert want >= Fraction(1, comb(G, m)) and got >= 0 and np.isfinite(got)
        if want >= Fraction(1, 10 ** 290):
            r = _ratio(got, want, G)
            print(f"m={m} x={x:.6f}: tail {float(want):.6e}, port error / bound {r:.5f}")
            assert r <= 1.0
        else:                                                 # below 1e-290: digits may go, the value may not rise
            assert Fraction(got) <= want * (1 + Fraction(gx.rel_bound(G)))


def test_port_limits():
    assert gx.reg_count(1) == 1 and gx.reg_count(63) == 1 and gx.reg_count(64) == 2 and gx.reg_count(127) == 2 and gx.reg_count(128) == 4
    assert gx.reg_count(gx.MAX_SIZE) == 64 and np.isnan(gx.tail_f64(5000, gx.MAX_SIZE + 1, 0.5))
    assert gx.tail_f64(50, 7, 0.0) == 1.0 and gx.tail_exact(50, 7, 0.0) == 1
    assert gx.tail_exact(9, 1, 1.0) == Fraction(1, 9) and gx.tail_f64(9, 1, 1.0) == pytest.approx(1 / 9, rel=1e-15)
    # a score no set reaches
    assert gx.tail_exact(10, 4, np.nextafter(1.0, 2.0)) == 0 and gx.tail_f64(10, 4, np.nextafter(1.0, 2.0)) == 0.0


@pytest.fixture(scope="module")
def sampled_null():
    sizes = [1, 15, 40, 250, 499]
    return sizes, gs.null(500, 180582, sizes, 20000)


def test_sampler_consistency(sampled_null):
    """The library's sampler against the exact tail: at each quantile of each side of each null row the count of null values
    at or beyond x is binomial(nsim, tail), so it lies within 4 sigma of nsim * tail."""
    sizes, null = sampled_null
    G, nsim, worst = 500, null.shape[1], 0.0
    for m, row in zip(sizes, null):
        for side in (+1, -1):
            part = row[row > 0] if side > 0 else -row[row < 0]
            for qt in (0.8, 0.95, 0.99, 0.999):
                x = side * float(np.quantile(part, qt, method="lower"))
                seen = int((row >= x).sum() if side > 0 else (row <= x).sum())
                p = float(gx.tail_exact(G, m, x))
                assert abs(gx.tail_f64(G, m, x) / p - 1) <= gx.rel_bound(G)
                z = abs(seen - nsim * p) / np.sqrt(nsim * p * (1 - p))
                print(f"m={m} side={side:+d} q={qt}: x={x:+.6f} seen {seen} expected {nsim * p:.1f} z={z:.2f}")
                assert 0 < p < 1 and z <= 4.0, (m, side, qt)
                worst = max(worst, z)
    print(f"worst of 40: {worst:.2f} sigma")


# ------------------------------------------------------------------ plumbing
def test_header_and_loader_name_the_same_entries():
    from gficf_amd import _gsea_exact_lib as lib

    text = open(os.path.join(ROOT, "include", "gficf_gsea_exact.h")).read()
    body = text[text.index("extern \"C\""):]
    declared = re.findall(r"\b(gficf_gsea_\w+)\s*\(([^;]*)\)\s*;", body)
    assert set(n for n, _ in declared) == set(lib.SIGNATURES) and len(declared) == 5
    for name, args in declared:
        n = 0 if args.strip() == "void" else args.count(",") + 1
        assert n == len(lib.SIGNATURES[name][1]), name
    assert "#define GFICF_GSEA_EXACT_ABI_VERSION 1" in text and lib.ABI_VERSION == 1
    for macro, value in (("MAX_G", lib.MAX_G), ("MAX_SIZE", lib.MAX_SIZE)):
        assert re.search(rf"#define\s+GFICF_GSEA_EXACT_{macro}\s+{value}\b", text), macro
    assert lib.MAX_SIZE >= 2048 and lib.MAX_SIZE == gx.MAX_SIZE and lib.MAX_G == 131072
    core = open(os.path.join(ROOT, "include", "gficf_hip.h")).read()
    assert re.search(r"#define\s+GFICF_HIP_ABI_VERSION\s+7\b", core)
    old = open(os.path.join(ROOT, "include", "gficf_gsea.h")).read()
    assert "#define GFICF_GSEA_ABI_VERSION 1" in old and "gficf_gsea_tail" not in old


def test_makefile_builds_the_library_with_the_others():
    csrc = os.path.join(ROOT, "gficf_amd", "csrc")
    build = subprocess.run(["make", "-n", "-B", "-C", csrc, "all"], capture_output=True, text=True, check=True).stdout.splitlines()
    link = [ln for ln in build if " -o ../libgficf_gsea_exact.so " in ln]
    assert len(link) == 1 and re.search(r"hipcc --offload-arch=gfx950 -shared -fPIC -o \.\./libgficf_gsea_exact\.so gsea_exact\.o -L\.\. -lgficf_hip\b",
                                        link[0])
    comp = [ln for ln in build if ln.endswith(" -o gsea_exact.o")]
    assert len(comp) == 1 and "-ffp-contract=off" in comp[0] and "--offload-arch=gfx950" in comp[0] and "fast-math" not in comp[0]
    assert build.index(link[0]) > max(i for i, ln in enumerate(build) if " -o ../libgficf_hip.so " in ln or ln.endswith(" -o gsea_exact.o"))
    assert len([ln for ln in build if " -o ../libgficf_gsea.so gsea.o " in ln]) == 1          # the sampled library keeps its own object
    clean = subprocess.run(["make", "-n", "-C", csrc, "clean"], capture_output=True, text=True, check=True).stdout
    assert re.search(r"^rm -f .*\bgsea_exact\.o\b.* \.\./libgficf_gsea_exact\.so\b", clean, re.M)


def test_loader(monkeypatch):
    from gficf_amd import _gsea_exact_lib as lib

    L = lib.load()
    assert isinstance(L, ctypes.CDLL) and lib.load() is L and L.gficf_gsea_exact_abi_version() == lib.ABI_VERSION
    for sym, (res, args) in lib.SIGNATURES.items():
        fn = getattr(L, sym)
        assert fn.restype is res and list(fn.argtypes) == list(args), sym
    assert os.path.basename(lib.LIB_PATH) == "libgficf_gsea_exact.so"
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert sorted(set(re.findall(r" T (gficf_[a-z0-9_]+)$", out, re.M))) == sorted(lib.SIGNATURES)
    # the status word and one reciprocal per position, whatever n is
    assert 8 * 20000 <= L.gficf_gsea_tail_workspace_bytes(20000, 0) == L.gficf_gsea_tail_workspace_bytes(20000, 125000) <= 8 * 20000 + 1024
    assert L.gficf_gsea_tail_workspace_bytes(lib.MAX_G, 1) > 0 and L.gficf_gsea_tail_workspace_bytes(lib.MAX_G + 1, 1) == 0
    assert L.gficf_gsea_tail_workspace_bytes(1, 1) == 0 and L.gficf_gsea_tail_workspace_bytes(10, -1) == 0
    monkeypatch.setattr(lib, "LIB_PATH", os.path.join(os.path.dirname(lib.LIB_PATH), "libgficf_gsea_exact_missing.so"))
    with pytest.raises(ImportError, match="not found: build it with"):
        lib.load()


def test_new_keywords():
    for fn in (gficf_amd.gsea, gficf_amd.fgsea, gficf_amd.runGSEA):
        p = inspect.signature(fn).parameters["exact"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False, fn.__name__
    assert list(inspect.signature(gficf_amd.gsea_tail).parameters) == ["G", "size", "es", "ctx"]
    assert list(inspect.signature(gficf_amd.gsea).parameters)[:9] == ["stats", "pathways_ptr", "pathways_rows", "nsim", "min_size", "max_size", "seed",
                                                                     "ret_null", "ctx"]
    with pytest.raises(TypeError):
        gficf_amd.gsea(np.ones((4, 1)), [0, 2], [0, 1], 10, 1, np.inf, 1, False, None, True)      # exact is keyword-only
    with pytest.raises(ValueError, match="pathways_ptr"):
        gficf_amd.gsea(np.ones((4, 1)), [0, 3], [0, 1], exact=True)
    with pytest.raises(ValueError, match="Please run clustcell function first"):
        gficf_amd.runGSEA({"gficf": None}, "none.gmt", exact=True)
    with pytest.raises(ValueError, match="int32 set sizes"):
        gficf_amd.gsea_tail(10, [1.5], [0.5])
    with pytest.raises(ValueError, match="at least 2"):
        gficf_amd.gsea_tail(1, [1], [0.5])
    with pytest.raises(ValueError):                                                                # shapes that do not broadcast
        gficf_amd.gsea_tail(10, [1, 2, 3], [0.5, 0.25])
    for fn in (gficf_amd.gsea, gficf_amd.runGSEA):
        assert "pval_exact" in fn.__doc__ and "sign" in fn.__doc__
    assert hasattr(gficf_amd.HipOps, "gsea_tail") and hasattr(gficf_amd.HipOps, "gsea_tail_sync") and hasattr(gficf_amd.HipOps, "gsea_tail_workspace_bytes")
