"""CPU: the GSEA oracle (tests/helpers/gsea_np.py) against itself, hand-derived values and an independent sampler; gmt parsing
and the argument errors of runGSEA; the exported surface of libgficf_gsea.so."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.helpers import gsea_np as gs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind", ["distinct", "ties", "zero_tail"])
def test_literal_and_position_forms_agree_bit_for_bit(kind):
    rng = np.random.default_rng({"distinct": 1, "ties": 2, "zero_tail": 3}[kind])
    for G in (10, 33, 257, 1000):
        stats = rng.normal(size=G)
        if kind == "ties":
            stats = np.round(stats * 2) / 2
        if kind == "zero_tail":
            stats = np.abs(stats)
            stats[rng.random(G) < 0.6] = 0.0
            stats[rng.random(G) < 0.1] = -0.0
        r = gs.ranks(stats)
        for m in sorted({1, 2, min(15, G - 1), G // 2, G - 1}):
            rows = rng.choice(G, m, replace=False)
            a = gs.es_literal(stats, rows)
            b = gs.es_positions(np.sort(r[rows]) + 1, G)
            assert a == b and np.signbit(a) == np.signbit(b), (G, m, a, b)
            assert b == gs.es_of_set(r[rows], G)


def test_order_breaks_ties_by_row_and_joins_the_zeros():
    assert gs.order_desc([0.0, 2.0, -0.0, 2.0, -1.0, 0.0]).tolist() == [1, 3, 0, 2, 5, 4]
    assert gs.ranks([0.0, 2.0, -0.0, 2.0, -1.0, 0.0]).tolist() == [2, 0, 3, 1, 5, 4]


def test_hand_derived_scores():
    G = 10
    stats = np.arange(G, 0, -1, dtype=np.float64)           # row g at position g
    assert gs.es_literal(stats, [0, 1, 2]) == 1.0
    assert gs.es_literal(stats, [7, 8, 9]) == -1.0
    assert gs.es_positions([1, 2, 3], G) == 1.0 and gs.es_positions([8, 9, 10], G) == -1.0
    for G in (10, 11, 33):
        stats = np.arange(G, 0, -1, dtype=np.float64)
        for s in range(1, G + 1):                            # one member at 1-based position s
            top, bottom = 1 - (s - 1) / (G - 1), -(s - 1) / (G - 1)
            want = top if 2 * (s - 1) < G - 1 else (0.0 if 2 * (s - 1) == G - 1 else bottom)
            assert gs.es_positions([s], G) == want
            assert gs.es_literal(stats, [s - 1]) == want
        assert gs.es_positions([(G + 1) // 2], G) == (0.0 if G % 2 else 1 - (G // 2 - 1) / (G - 1))
    # G = 2m, m a power of two (every quotient exact).  Alternate members: the walk never leaves [0, 1/m] (odd positions) or
    # [-1/m, 0] (even ones), so ES = +-1/m, not 0.  The tie maxP = -minP needs a walk that reaches both: members in mirrored
    # pairs (hit, miss, miss, hit) reach +1/m and -1/m, and ES is exactly 0.0.
    for m in (2, 4, 16, 64):
        assert gs.es_positions(np.arange(1, 2 * m + 1, 2), 2 * m) == 1 / m
        assert gs.es_positions(np.arange(2, 2 * m + 1, 2), 2 * m) == -1 / m
        k = np.arange(m // 2)
        mirrored = np.sort(np.concatenate([4 * k + 1, 4 * k + 4]))
        assert gs.es_positions(mirrored, 2 * m) == 0.0 and not np.signbit(gs.es_positions(mirrored, 2 * m))
        assert gs.es_literal(np.arange(2 * m, 0, -1.0), mirrored - 1) == 0.0


def test_mix32_hand_values_and_bijection():
    assert int(gs.mix32(0)) == 0
    x = 1                                                    # the rounds by hand, in Python integers
    x ^= x >> 16; x = x * 0x7FEB352D & 0xFFFFFFFF; x ^= x >> 15; x = x * 0x846CA68B & 0xFFFFFFFF; x ^= x >> 16
    assert int(gs.mix32(1)) == x
    v = gs.mix32(np.arange(1 << 16, dtype=np.uint64) * np.uint64(65537))
    assert len(np.unique(v)) == 1 << 16 and v.max() < 2 ** 32


@pytest.mark.parametrize("G", [1, 2, 33, 64, 1000])
def test_perm_is_a_bijection(G):
    for seed, j in ((180582, 0), (180582, 7), (0, 0), (2 ** 32 - 1, 2 ** 31)):
        p = gs.perm(G, seed, j)
        assert p.dtype == np.int32 and np.array_equal(np.sort(p), np.arange(G))
    if G >= 33:
        assert not np.array_equal(gs.perm(G, 180582, 0), gs.perm(G, 180582, 1))
        assert not np.array_equal(gs.perm(G, 180582, 0), gs.perm(G, 180583, 0))


NULL_CASES = {33: (1, 5, 16, 32), 64: (15, 32), 1000: (15, 100, 500), 4097: (15, 64, 2000)}


@pytest.mark.parametrize("G", sorted(NULL_CASES))
def test_null_matches_an_independent_sampler(G):
    """The means of the non-negative and of the non-positive null values against the same means over sets drawn by NumPy's
    generator: |difference| <= 5 standard errors (the NumPy sample's variance, both counts)."""
    nsim, sizes = 2000, NULL_CASES[G]
    mine = gs.null(G, 180582, sizes, nsim)
    rng = np.random.default_rng(20240607 + G)
    for d, m in enumerate(sizes):
        theirs = np.array([gs.es_of_set(rng.choice(G, m, replace=False), G) for _ in range(nsim)])
        for side in (1, -1):
            a, b = mine[d][side * mine[d] >= 0], theirs[side * theirs >= 0]
            assert len(a) > 100 and len(b) > 100
            se = np.sqrt(b.var(ddof=1) * (1 / len(a) + 1 / len(b)))
            z = abs(a.mean() - b.mean()) / se
            print(f"G={G} m={m} side={side}: {z:.2f} sigma")
            assert z <= 5.0, (G, m, side, z)


def test_null_value_depends_on_seed_j_G_m_only():
    a = gs.null(64, 5, (15, 32), 6)
    assert np.array_equal(gs.null(64, 5, (32,), 4)[0], a[1, :4])
    assert np.array_equal(gs.null(64, 5, (15,), 3, j0=3)[0], a[0, 3:])


def test_stats_of_hand_values():
    s = gs.stats_of(0.5, [0.25, 0.5, 0.75, -0.5, -0.25, 0.0])
    assert (s["nGeEs"], s["nLeEs"], s["nGeZero"], s["nLeZero"]) == (2, 5, 4, 3)
    assert s["geZeroMean"] == 1.5 / 4 and s["leZeroMean"] == -0.75 / 3
    assert s["nes"] == 0.5 / (1.5 / 4) and s["pval"] == min(6 / 4, 3 / 5)
    s = gs.stats_of(-0.5, [0.25, 0.5, 0.75, -0.5, -0.25, 0.0])
    assert s["nes"] == -0.5 / 0.25 and s["pval"] == min(2 / 4, 7 / 5)
    assert np.isinf(gs.stats_of(-0.5, [0.25, 0.5])["nes"]) or np.isnan(gs.stats_of(-0.5, [0.25, 0.5])["nes"])


# ------------------------------------------------------------------------------------------------ the Python surface
def test_gmt_pathways(tmp_path):
    import gficf_amd

    f = tmp_path / "sets.gmt"
    f.write_text("A\thttp://a\tg1\tg2\tg3\nEMPTY\tnone\nB\tdescr\tg2\tg9\t\nC\tdescr\tzz\n")
    got = gficf_amd.gmt_pathways(str(f), verbose=False)
    assert got == {"A": ["g1", "g2", "g3"], "B": ["g2", "g9"], "C": ["zz"]}
    assert list(got) == ["A", "B", "C"]
    gene_map = {"g1": ["E1"], "g2": ["E2a", "E2b"], "g3": ["E1"], "g9": "E9"}
    got = gficf_amd.gmt_pathways(str(f), convertToEns=True, verbose=False, gene_map=gene_map)
    assert got == {"A": ["E1", "E2a", "E2b"], "B": ["E2a", "E2b", "E9"]}          # C maps to nothing: dropped
    assert gficf_amd.gmt_pathways(str(f), convertHu2Mm=True, verbose=False, gene_map=gene_map) == got
    for kw in ({"convertToEns": True}, {"convertHu2Mm": True}, {"convertToEns": True, "convertHu2Mm": True}):
        with pytest.raises(NotImplementedError, match="gene_map"):
            gficf_amd.gmt_pathways(str(f), verbose=False, **kw)


def test_run_gsea_argument_errors(tmp_path):
    import gficf_amd

    f = tmp_path / "sets.gmt"
    f.write_text("A\tx\tg1\tg2\n")
    with pytest.raises(ValueError, match="Please run clustcell function first"):
        gficf_amd.runGSEA({"gficf": None}, str(f))
    data = {"cluster.gene.rnk": np.ones((4, 2))}
    with pytest.raises(NotImplementedError, match="GSVA"):
        gficf_amd.runGSEA(data, str(f), method="GSVA", verbose=False)
    with pytest.raises(NotImplementedError, match="gene_map"):
        gficf_amd.runGSEA(data, str(f), convertToEns=True, verbose=False, gene_names=["g1", "g2", "g3", "g4"])
    with pytest.raises(ValueError, match="method"):
        gficf_amd.runGSEA(data, str(f), method="other", verbose=False)
    with pytest.raises(ValueError, match="gene_names"):
        gficf_amd.runGSEA(data, str(f), verbose=False)
    with pytest.raises(ValueError, match="pathways_ptr"):
        gficf_amd.gsea(np.ones((4, 1)), [0, 3], [0, 1])
    import inspect

    sig = inspect.signature(gficf_amd.runGSEA)
    assert list(sig.parameters)[:11] == ["data", "gmt_file", "nsim", "convertToEns", "convertHu2Mm", "nt", "minSize", "maxSize", "verbose",
                                         "seed", "method"]
    assert sig.parameters["nsim"].default == 1000 and sig.parameters["minSize"].default == 15 and sig.parameters["seed"].default == 180582
    assert sig.parameters["convertToEns"].default is False        # the one default that differs from the reference


def _header_functions():
    src = open(os.path.join(ROOT, "include", "gficf_gsea.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gficf_[a-z0-9_]+)\s*\(", src)))


def test_gsea_library_exports_exactly_its_header():
    from gficf_amd import _gsea_lib

    names = _header_functions()
    assert len(names) == 7
    assert sorted(_gsea_lib.SIGNATURES) == names
    L = _gsea_lib.load()
    assert L.gficf_gsea_abi_version() == 1
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", _gsea_lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert sorted(set(re.findall(r" T (gficf_[a-z0-9_]+)$", out, re.M))) == names
    # the batch: min(nsim, 1024, 2^22 / G), at least 1, and at least 32 at the largest G
    assert L.gficf_gsea_perm_batch(65, 10) == 10 and L.gficf_gsea_perm_batch(65, 5000) == 1024
    assert L.gficf_gsea_perm_batch(8225, 5000) == (1 << 22) // 8225 and L.gficf_gsea_perm_batch(131072, 5000) == 32
    assert L.gficf_gsea_perm_batch(0, 5) == 0 and L.gficf_gsea_perm_batch(5, 0) == 0
    # bounded in nsim but for the null table (8 B per size and permutation)
    a, b = (L.gficf_gsea_workspace_bytes(20000, 25, 5000, 10 ** 6, 400, n) for n in (1000, 100000))
    assert 0 < a and b - a <= 400 * 99000 * 8 + 4096
    assert L.gficf_gsea_workspace_bytes(131073, 2, 5, 50, 1, 10) == 0
