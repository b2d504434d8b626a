"""No GPU: the surface of libgficf_sparse_query.so (header, loader, symbols, Makefile), the NumPy oracle of the query search
(tests/helpers/sparse_query_oracle.py) against a brute-force loop and under a permuted summation order, its comparison rule, the
shape rule, everything the Python mirror decides before the first call into the library, and the condition on the INPUTS of the
exact device test (tests/helpers/sparse_query_par.py): each deliberately wrong summation order changes the f32 bits of at least
three query -> twin distances at every (metric, tile width)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import gficf_amd
from gficf_amd import GficfError, _sparse_knn_lib, _sparse_query_lib
from tests.helpers import sparse_knn_cases as sc
from tests.helpers import sparse_knn_oracle as so
from tests.helpers import sparse_query_oracle as qo
from tests.helpers import sparse_query_par as qp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TQS = (8, 4, 2, 1)
MIN_CHANGED = 3                                                # the floor of tests/test_sparse_knn_par_cpu.py


# ------------------------------------------------------------------------------------------------ the library's surface
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(re.findall(r" T (gficf_[a-z0-9_]+)$", out, re.M)))


def test_header_and_loader_name_the_same_entries():
    text = open(os.path.join(ROOT, "include", "gficf_sparse_query.h")).read()
    body = re.sub(r"/\*.*?\*/", "", text[text.index("extern \"C\""):], flags=re.S)
    declared = {m.group(1): m.group(2) for m in re.finditer(r"\b(gficf_sparse_query_\w+)\s*\(([^)]*)\)\s*;", body)}
    assert set(declared) == set(_sparse_query_lib.SIGNATURES) and len(declared) == 6
    for name, args in declared.items():
        n = 0 if args.strip() == "void" else args.count(",") + 1
        assert n == len(_sparse_query_lib.SIGNATURES[name][1]), name
    assert "#define GFICF_SPARSE_QUERY_ABI_VERSION 1" in text and _sparse_query_lib.ABI_VERSION == 1
    assert '#include "gficf_sparse_knn.h"' in text            # the contract is stated by reference to it
    core = open(os.path.join(ROOT, "include", "gficf_hip.h")).read()
    assert re.search(r"#define\s+GFICF_HIP_ABI_VERSION\s+7\b", core)
    L = _sparse_query_lib.load()
    assert L.gficf_sparse_query_abi_version() == 1
    if shutil.which("nm"):
        assert _exported(_sparse_query_lib.LIB_PATH) == sorted(_sparse_query_lib.SIGNATURES)
        _sparse_knn_lib.load()
        assert _exported(_sparse_knn_lib.LIB_PATH) == sorted(_sparse_knn_lib.SIGNATURES) and len(_sparse_knn_lib.SIGNATURES) == 6
    wb = L.gficf_sparse_query_workspace_bytes
    # the f32 copies of both matrices' values, two scalars per cell of each, one list of k keys per query and slice (2 at M = 1000)
    assert wb(5000, 53000, 1_000_000, 1000, 20_000, 16) >= 4 * 1_020_000 + 16 * 54000 + 8 * 16 * 1000 * 2
    assert wb(5000, 53000, 1_000_000, 0, 0, 16) > 0
    for bad in ((0, 10, 5, 3, 2, 2), (_sparse_knn_lib.LDS_FLOATS + 1, 10, 5, 3, 2, 2), (10, 0, 0, 3, 2, 2), (10, 10, 5, -1, 0, 2), (10, 10, 5, 3, 2, 129),
                (10, 10, 5, 3, 2, 0), (10, 10, -1, 3, 2, 2), (10, 10, 5, 3, -1, 2)):
        assert wb(*bad) == 0, bad


def test_makefile_builds_links_and_cleans_the_add_on():
    mk = open(os.path.join(ROOT, "gficf_amd", "csrc", "Makefile")).read()
    addons = re.search(r"^ADDONS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert "sparse_query" in addons and "sparse_knn" in addons
    # every add-on links the core the same way, and nothing else
    assert re.search(r"^\$\(ADDON_OUT\): \.\./libgficf_%\.so: %\.o \$\(OUT\)\n\t.*-lgficf_hip \$\(ADDON_LIBS\)", mk, re.M)
    assert not re.search(r"libgficf_sparse_query\.so:\s*ADDON_LIBS", mk)
    dep = re.search(r"^sparse_query\.o:(.*\.h.*)$", mk, re.M).group(1)
    assert "gficf_sparse_query.h" in dep and "sparse_knn_tiles.h" in dep and "addon_status.h" in dep
    assert re.search(r"^sparse_query\.o: HIPFLAGS \+= -ffp-contract=off$", mk, re.M)
    assert "sparse_knn_tiles.h" in re.search(r"^sparse_knn\.o:(.*\.h.*)$", mk, re.M).group(1)
    assert re.search(r"^sparse_knn\.o: HIPFLAGS \+= -ffp-contract=off$", mk, re.M)
    assert re.search(r"^clean:\n\trm -f .*\$\(ADDONS:%=%\.o\) \$\(ADDON_OUT\)", mk, re.M)
    assert "libgficf_sparse_query.so" in mk[:mk.index("HIPCC")]   # the head comment names it
    tiles = open(os.path.join(ROOT, "gficf_amd", "csrc", "sparse_knn_tiles.h")).read()
    for name in ("sk_tile_queries", "sk_slices", "k_sk_prepare", "struct SkArgs", "k_sk_tiles", "k_sk_merge", "sk_tile_lds", "sk_launch_tq"):
        assert name in tiles, name
    for src in ("sparse_knn.hip", "sparse_query.hip"):
        text = open(os.path.join(ROOT, "gficf_amd", "csrc", src)).read()
        assert '#include "sparse_knn_tiles.h"' in text and "__global__" not in text, src


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("metric", qo.METRICS)
def test_oracle_against_a_brute_force_loop(metric):
    train, Q = qo.pair_case(30, 40, 9, 5, 12, 1)
    want = qo.oracle(train, Q, metric, 8)
    assert want["q"].shape == (9, 40)
    idx, dist = qo.brute_force(train, Q, metric, 8)
    assert qo.compare({"idx": idx, "dist": dist}, want, metric) == []
    assert np.array_equal(idx, want["idx"])


def test_oracle_has_no_self_rule():
    """A query equal to a training cell is computed like every other pair: 0 under euclidean, and the square oracle's diagonal
    write does not reach the block."""
    train, Q = qo.pair_case(30, 40, 9, 5, 12, 1)
    Q = sp.hstack([Q, train[:, 4]], format="csc")
    for metric in qo.METRICS:
        q, _ = qo.q_and_scale(train, Q, metric)
        assert q.shape == (10, 40) and q[9, 4] <= 2.0 ** -51 and (q[:9] > 1e-6).all()
        assert qo.table(q, metric, 1)[0][9, 0] == 5


def test_comparison_rule_catches_a_lost_neighbour_and_a_wrong_distance():
    train, Q = qo.pair_case(30, 40, 200, 5, 12, 2)
    want = qo.oracle(train, Q, "euclidean", 8)
    far = qo.table(want["q"], "euclidean", 9)
    lost = {"idx": np.delete(far[0], 3, axis=1), "dist": np.delete(far[1], 3, axis=1)}         # every row skips its 4th neighbour
    with pytest.raises(AssertionError, match="differ from the oracle"):
        qo.compare(lost, want, "euclidean")
    off = {"idx": want["idx"].copy(), "dist": want["dist"].copy()}
    off["dist"][5, 7] *= 1 + 2.0 ** -20
    with pytest.raises(AssertionError, match="tolerance"):
        qo.compare(off, want, "euclidean")
    out = {"idx": want["idx"].copy(), "dist": want["dist"]}
    out["idx"][0, 0] = 41                                                                     # no training cell
    with pytest.raises(AssertionError):
        qo.compare(out, want, "euclidean")
    assert qo.compare({"idx": want["idx"], "dist": want["dist"]}, want, "euclidean") == []


@pytest.mark.parametrize("metric", qo.METRICS)
def test_the_seeds_take_the_second_branch_in_no_row(metric):
    """The cases of the device tests under ANOTHER summation order (the genes renumbered): the oracle's own table passes the rule
    against the oracle with 0 rows in the second branch of rule 4, so a device row there is the device's doing."""
    G, N, M, lo, hi, seed = qo.BASIC
    train, Q = qo.pair_case(G, N, M, lo, hi, seed)
    lengths = np.concatenate([np.diff(train.indptr), np.diff(Q.indptr)])
    assert lengths.min() >= 12 and lengths.max() <= 40
    cases = [(train, Q, k) for k in qo.BASIC_KS]
    cases += [(*qo.seam_case(g, 9), qo.SEAM_K) for g in qo.SEAM_GS]
    for train, Q, k in cases:
        want = qo.oracle(train, Q, metric, k)
        other = qo.oracle(*qo.permuted(train, Q), metric, k)
        assert qo.compare({"idx": other["idx"], "dist": other["dist"]}, want, metric) == [], (train.shape, k)


def test_seam_cases_store_the_end_rows():
    for G in qo.SEAM_GS:
        train, Q = qo.seam_case(G, 5)
        assert train.shape == (G, qo.SEAM_N) and Q.shape == (G, 5)
        for A, c in ((train, 0), (Q, 4)):
            r = A.indices[A.indptr[c]:A.indptr[c + 1]]
            assert r[0] == 0 and r[-1] == G - 1
        assert (train.T @ Q).nnz > 20                                  # cells share genes at every G


# ------------------------------------------------------------------------------------------------ the shape rule
def test_shape_rule():
    top = gficf_amd.find_nn_sparse_query_shape(1, 300, 37, 16)
    assert top["tile_queries"] == 8 and top["max_genes"] == _sparse_knn_lib.LDS_FLOATS
    for G, tq in ((4096, 8), (4097, 4), (8192, 4), (8193, 2), (16384, 2), (16385, 1), (32768, 1)):
        assert gficf_amd.find_nn_sparse_query_shape(G, 40, 3, 10)["tile_queries"] == tq
        assert gficf_amd.find_nn_sparse_shape(G, 40, 10)["tile_queries"] == tq                 # one rule for both searches
    with pytest.raises(GficfError) as e:
        gficf_amd.find_nn_sparse_query_shape(32769, 40, 3, 10)
    assert e.value.status == "GFICF_ERR_UNSUPPORTED" and "32768" in str(e.value)
    # the slices: sk_slices(M, N, tq): enough workgroups to fill 256 CUs, no slice under 256 candidates, 32 at the most
    for N, M, want in ((8200, 5, 32), (8200, 8, 32), (8200, 9, 32), (8200, 8 * 256, 1), (53000, 1000, 3), (150, 37, 1), (600, 150, 2),
                       (255, 1, 1), (512, 1, 2), (40, 0, 1)):
        assert gficf_amd.find_nn_sparse_query_shape(300, N, M, 1)["slices"] == want, (N, M)
    for bad, status in (((300, 0, 5, 1), "GFICF_ERR_INVALID_ARG"), ((300, 10, 5, 11), "GFICF_ERR_INVALID_ARG"), ((300, 10, -1, 1), "GFICF_ERR_INVALID_ARG"),
                        ((300, 600, 5, 129), "GFICF_ERR_UNSUPPORTED"), ((300, 600, 5, 0), "GFICF_ERR_INVALID_ARG")):
        with pytest.raises(GficfError) as e:
            gficf_amd.find_nn_sparse_query_shape(*bad)
        assert e.value.status == status, bad


# ------------------------------------------------------------------------------------------------ the mirror's checks
def test_find_nn_sparse_query_argument_checks():
    train, Q = qo.pair_case(30, 40, 9, 5, 12, 1)
    with pytest.raises(ValueError, match="metric must be one of"):
        gficf_amd.find_nn_sparse_query(train, Q, 5, metric="chebyshev")
    with pytest.raises(ValueError, match="k must be at least 1"):
        gficf_amd.find_nn_sparse_query(train, Q, 0)
    with pytest.raises(ValueError, match="Q must be a 2-d"):
        gficf_amd.find_nn_sparse_query(train, np.zeros(5), 2)
    with pytest.raises(ValueError, match="M_train is 30 x 0"):
        gficf_amd.find_nn_sparse_query(sp.csc_matrix((30, 0)), Q, 2)
    with pytest.raises(ValueError, match=r"Q has 29 rows \(genes\), M_train has 30"):
        gficf_amd.find_nn_sparse_query(train, Q[:29], 2)
    x = Q.data.copy()
    x[3] = np.nan
    with pytest.raises(ValueError, match="finite as float32"):
        gficf_amd.find_nn_sparse_query(train, sp.csc_matrix((x, Q.indices, Q.indptr), shape=Q.shape), 5)
    rows = Q.indices.copy()
    b = Q.indptr[np.argmax(np.diff(Q.indptr) >= 2)]
    rows[b], rows[b + 1] = rows[b + 1], rows[b]
    unsorted = sp.csc_matrix((Q.data, rows, Q.indptr), shape=Q.shape)
    unsorted.has_sorted_indices = True                                    # a caller's promise that does not hold
    with pytest.raises(ValueError, match="strictly ascending"):
        gficf_amd.find_nn_sparse_query(train, unsorted, 5)
    with pytest.raises(ValueError, match="classes must hold one label per column of train: 40"):
        gficf_amd.knn_classify_sparse(train, Q, np.zeros(39))
    with pytest.raises(ValueError, match="rows"):
        gficf_amd.knn_classify_sparse(train, Q[:29], np.zeros(40))


def test_umap_transform_sparse_argument_checks():
    train, Q = qo.pair_case(30, 40, 9, 5, 12, 1)
    model = {"space": "gficf", "embedding": np.zeros((40, 2)), "metric": "euclidean", "n_neighbors": 5, "n_epochs": 30, "seed": 1, "a": 1.0, "b": 1.0}
    with pytest.raises(ValueError, match="runReductionSparse.*umap_transform"):
        gficf_amd.umap_transform_sparse(Q, dict(model, space=None), train)
    with pytest.raises(ValueError, match="40 x 2: M_train is not what the model was trained on"):
        gficf_amd.umap_transform_sparse(Q, dict(model, embedding=np.zeros((39, 2))), train)
    with pytest.raises(ValueError, match="metric must be one of"):
        gficf_amd.umap_transform_sparse(Q, dict(model, metric="chebyshev"), train)
    with pytest.raises(ValueError, match=r"Q has 29 rows"):
        gficf_amd.umap_transform_sparse(Q[:29], model, train)
    with pytest.raises(ValueError, match="init must be 'weighted' or an M x 2 array"):
        gficf_amd.umap_transform_sparse(Q, model, train, init="random")
    with pytest.raises(ValueError, match="9 x 2"):
        gficf_amd.umap_transform_sparse(Q, model, train, init=np.zeros((8, 2)))
    with pytest.raises(ValueError, match="finite"):
        gficf_amd.umap_transform_sparse(Q, model, train, init=np.full((9, 2), np.nan))
    none = gficf_amd.umap_transform_sparse(sp.csc_matrix((30, 0)), model, train, ret_extra=True)      # nothing to place: no device needed
    assert none["embedding"].shape == (0, 2) and none["idx"].shape == (0, 5) and none["idx"].dtype == np.int32
    assert set(none) == {"embedding", "idx", "dist", "w", "sigma", "rho", "init"}
    assert gficf_amd.knn_classify_sparse(train, sp.csc_matrix((30, 0)), np.arange(40) % 3).shape == (0,)


def test_refusals_of_embed_new_cells_sparse_and_classify_cells():
    x = sp.csc_matrix((5, 2))
    with pytest.raises(NotImplementedError, match="tsne"):
        gficf_amd.embedNewCellsSparse({"reduction": "tsne", "uwot": None}, x, verbose=False)
    with pytest.raises(ValueError, match="runReductionSparse"):
        gficf_amd.embedNewCellsSparse({"reduction": "tumap"}, x, verbose=False)
    with pytest.raises(ValueError, match="embedNewCells") as e:
        gficf_amd.embedNewCellsSparse({"reduction": "tumap", "uwot": {"embedding": None}}, x, verbose=False)
    assert "embedNewCellsSparse" in str(e.value) and "data['pca']" in str(e.value)
    sparse_model = {"reduction": "tumap", "uwot": {"space": "gficf"}, "gficf": sp.csc_matrix((3, 4)), "w": np.ones(3), "genes": np.arange(3)}
    with pytest.raises(TypeError, match=r"embedNewCellsSparse: unknown argument\(s\) \['perplexity'\]"):
        gficf_amd.embedNewCellsSparse(dict(sparse_model), x, verbose=False, perplexity=3)
    with pytest.raises(ValueError, match="needs data\\['gficf'\\]"):
        gficf_amd.embedNewCellsSparse(dict(sparse_model, gficf=None), x, verbose=False)
    with pytest.raises(ValueError, match="one row of x for every kept gene"):
        gficf_amd.embedNewCellsSparse(dict(sparse_model), x, genes=np.arange(2), verbose=False)
    with pytest.raises(ValueError, match="x has 5 rows"):
        gficf_amd.embedNewCellsSparse(dict(sparse_model, genes=np.array([0, 1, 7])), x, verbose=False)
    # embedNewCells keeps refusing the sparse model, and now says where to go
    with pytest.raises(NotImplementedError, match="runReductionSparse") as e:
        gficf_amd.embedNewCells({"uwot": {"space": "gficf"}, "reduction": "tumap", "pca": None}, x, verbose=False)
    assert "embedNewCellsSparse" in str(e.value)
    assert "embedNewCellsSparse" in gficf_amd.runReductionSparse.__doc__
    # classify_cells: a third method; an unknown one is still refused, and "gficf" needs the new cells' columns
    import pandas as pd

    assert gficf_amd.api.CLASSIFY_METHODS == ("PCA", "embedded", "gficf")
    emb = pd.DataFrame({"X": [0.0, 1.0], "Y": [0.0, 1.0], "predicted": pd.Categorical(["NO", "YES"], categories=["NO", "YES"])})
    with pytest.raises(ValueError, match="method must be one of"):
        gficf_amd.classify_cells({"embedded": emb}, ["a"], method="gficf.pred")
    with pytest.raises(ValueError, match="embedNewCellsSparse"):
        gficf_amd.classify_cells({"embedded": emb}, ["a"], method="gficf")
    with pytest.raises(ValueError, match="embed first"):
        gficf_amd.classify_cells({"embedded": emb[["X", "Y"]]}, ["a"], method="gficf")


def test_exports():
    for name in ("find_nn_sparse_query", "find_nn_sparse_query_shape", "umap_transform_sparse", "knn_classify_sparse", "embedNewCellsSparse"):
        assert callable(getattr(gficf_amd, name)), name
    for name in ("sparse_query_workspace_bytes", "sparse_query", "sparse_query_sync"):
        assert callable(getattr(gficf_amd.HipOps, name)), name


# ------------------------------------------------------------------------------------------------ the inputs of the exact device test
@pytest.mark.parametrize("tq", TQS)
def test_the_split_holds_what_the_device_tests_rely_on(tq):
    G = sc.tile_genes()[tq]
    c, s = sc.case(G), qp.split(G)
    train, Q = s["train"], s["Q"]
    N, M = train.shape[1], Q.shape[1]
    assert gficf_amd.find_nn_sparse_query_shape(G, N, M, 16)["tile_queries"] == tq
    assert N + len(c["pairs"]) + len(c["mpairs"]) == c["M"].shape[1] and N >= 129          # k = 128 has its candidates
    assert M % 2 == 1 and M == len(c["pairs"]) + len(c["mpairs"]) + len(s["duplicates"])
    dense_t, dense_q = train.toarray(), Q.toarray()
    for qpos, tid in s["duplicates"]:
        assert np.array_equal(dense_q[:, qpos], dense_t[:, tid])
    long_dups = [(q, t) for q, t in s["duplicates"] if Q.indptr[q + 1] - Q.indptr[q] >= min(255, G)]
    assert len(long_dups) >= 12 or G < 255
    assert Q.indptr[s["empty"] + 1] == Q.indptr[s["empty"]] and (np.diff(train.indptr) == 0).any()
    for twins in (s["twins"], s["mtwins"]):
        for qpos, tid in twins:                                                               # a twin: the same rows, other values
            a, b = slice(Q.indptr[qpos], Q.indptr[qpos + 1]), slice(train.indptr[tid], train.indptr[tid + 1])
            assert np.array_equal(Q.indices[a], train.indices[b]) and not np.array_equal(Q.data[a], train.data[b])
    for metric in qp.METRICS:                                                                 # and its twin is a query's nearest but for duplicates
        tw = s["mtwins"] if metric == "manhattan" else s["twins"]
        idx, _ = qp.table(qp.contract(G, metric), 16)
        assert all(tid + 1 in idx[qpos] for qpos, tid in tw)


@pytest.mark.parametrize("metric", qp.METRICS)
@pytest.mark.parametrize("tq", TQS)
def test_the_amplifier_discriminates(tq, metric):
    """Every wrong order, in every sum or in the pair sums alone, changes the f32 bits of at least MIN_CHANGED query -> twin
    distances, although only one direction of a pair is a query here."""
    G = sc.tile_genes()[tq]
    s = qp.split(G)
    twins = s["mtwins"] if metric == "manhattan" else s["twins"]
    want = qp.contract(G, metric)[twins[:, 0], twins[:, 1]].view(np.uint32)
    assert np.array_equal(qp.twin_distances(s["train"], s["Q"], metric, twins).view(np.uint32), want)
    for scope in ("all", "pair"):
        for variant in qp.VARIANTS:
            got = qp.twin_distances(s["train"], s["Q"], metric, twins, variant, scope).view(np.uint32)
            changed = int((got != want).sum())
            print(f"TQ {tq} G {G} {metric} {variant} in {scope} sums: {changed} of {len(twins)} query -> twin distances change")
            assert changed >= MIN_CHANGED, (variant, scope, changed)


@pytest.mark.parametrize("metric", qp.METRICS)
def test_duplicates_under_the_contract(metric):
    """What the header says of a query equal to a training cell, on the restatement: exactly 0 under euclidean and manhattan, a
    value in [0, 2^-51] under cosine and correlation (not always 0); 1 for the empty query under those two."""
    G = sc.tile_genes()[8]
    s, d = qp.split(G), qp.contract(G, metric)
    dup = np.array([(q, t) for q, t in s["duplicates"] if q != s["empty"]])
    own = d[dup[:, 0], dup[:, 1]].astype(np.float64)
    if metric in ("euclidean", "manhattan"):
        assert (own == 0).all()
    else:
        assert (own >= 0).all() and (own <= 2.0 ** -51).all()
        assert (d[s["empty"]] == 1).all()
