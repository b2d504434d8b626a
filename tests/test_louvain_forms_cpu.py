"""tests/helpers/louvain_forms.py: every form tests/test_louvain_paths_gpu.py sends to the device is, in 2^-32 fixed point, the graph it
was made from — the same matrix after summing duplicates — with positive entries, symmetric sums and the row lengths asked for.  With that
shown here, on the CPU, two forms giving different labels on the GPU is the library's fault and not the test's.  The kNN -> Jaccard graphs
of the GPU tests need the device; a stand-in of the same row lengths takes their place (the generators never look at more than the
structure and the weights)."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.helpers import louvain_forms as lf
from tests.test_louvain_gpu import hub_graph


def check_form(Q, form, lengths=None):
    indptr, indices, x = form
    N = Q.shape[0]
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and x.dtype == np.float64
    assert indptr[0] == 0 and indptr[-1] == len(indices) == len(x) and (np.diff(indptr) >= 0).all()
    assert (x > 0).all() and (x <= 2.0 ** 20).all()                       # what k_lv_fix accepts, and no entry the kernels could skip
    assert np.array_equal(np.rint(x * lf.SCALE), x * lf.SCALE)            # whole fixed-point units: llrint rounds nothing
    M = lf.fixed_point_matrix(indptr, indices, x, N)
    assert lf.same_graph(M, lf.fixed_point_matrix(*lf.canonical(Q), N))
    assert lf.same_graph(M, M.T.tocsc())                                  # sort_indices is part of fixed_point_matrix; .T.tocsc() comes sorted
    if lengths is not None:
        assert np.array_equal(np.diff(indptr), lengths)
    return indptr


def graphs():
    yield "standin_g1", lf.quantise(lf.standin_knn_graph(3000, 15, 1))
    yield "standin_g2", lf.quantise(lf.standin_knn_graph(6000, 30, 2))
    yield "hubs", lf.quantise(hub_graph())
    yield "many_hubs", lf.quantise(lf.many_hubs_graph()[0])
    yield "components", lf.quantise(lf.components_graph()[0])


GRAPHS = dict(graphs())


def test_quantise():
    A = lf.standin_knn_graph(500, 10, 3)
    B = (A + sp.identity(500, format="csc") * 0.3).tocsc()
    Q = lf.quantise(B)
    assert Q.diagonal().sum() == 0 and Q.nnz == A.nnz and np.array_equal(Q.indices, A.indices)
    units = Q.data / lf.QUANT
    assert np.array_equal(units, np.rint(units)) and units.min() >= 1 and np.abs(Q.data - A.data).max() <= lf.QUANT / 2
    tiny = A.copy()
    tiny.data[:] = 1e-9
    assert (lf.quantise(tiny).data == lf.QUANT).all()
    lop = A.copy()
    lop.data[0] += 0.25
    with pytest.raises(AssertionError):
        lf.quantise(lop)


@pytest.mark.parametrize("name", list(GRAPHS))
def test_shuffle_keeps_the_entries_and_moves_them(name):
    Q = GRAPHS[name]
    indptr, indices, x = lf.form_shuffle(Q, np.random.default_rng(1))
    check_form(Q, (indptr, indices, x), np.diff(Q.indptr))
    assert not np.array_equal(indices, Q.indices)                         # it is not the sorted form
    plain = lf.cut_rows(Q, lf.parts_uniform(Q, 1), np.random.default_rng(1), shuffle=False)
    assert np.array_equal(plain[1], Q.indices) and np.array_equal(plain[2], Q.data)


@pytest.mark.parametrize("name,factor", [("standin_g1", 3), ("standin_g2", 3), ("standin_g1", 12), ("standin_g2", 12), ("standin_g1", 90),
                                         ("standin_g1", 300)])
def test_uniform_cut(name, factor):
    Q = GRAPHS[name]
    form = lf.form_uniform(Q, factor, np.random.default_rng(factor))
    check_form(Q, form, np.diff(Q.indptr) * factor)
    # uneven parts: the entries of one element are not all alike, so a dropped or doubled one changes the sum
    x = form[2][:form[0][1]]
    assert len(np.unique(x)) > len(x) // 2


def test_every_row_beyond_the_last_edge():
    Q = lf.quantise(lf.standin_knn_graph(300, 6, 5))                     # rows of 6 to about 20 entries
    deg = np.diff(Q.indptr)
    assert deg.min() * 300 <= 4096 < deg.max() * 300
    indptr = check_form(Q, lf.form_all_big(Q, 300, np.random.default_rng(2)), np.maximum(300, -(-4097 // deg)) * deg)
    assert lf.class_counts(indptr)["big"] == 300 and np.diff(indptr).min() > 4096


def test_parts_are_positive_at_the_smallest_weight():
    Q = GRAPHS["standin_g1"].copy()
    Q.data[:] = lf.QUANT                                                  # 2^16 units each
    form = lf.form_uniform(Q, 300, np.random.default_rng(0))
    check_form(Q, form, np.diff(Q.indptr) * 300)
    with pytest.raises(AssertionError):
        lf.cut_rows(Q, lf.parts_uniform(Q, 70000), np.random.default_rng(0))


def test_mixed_factors_reach_every_class():
    Q = GRAPHS["standin_g1"]
    rng = np.random.default_rng(4)
    indptr = check_form(Q, lf.form_mixed(Q, rng))
    counts = lf.class_counts(indptr)
    assert all(counts[c] > 0 for c in lf.CLASS_NAMES), counts


def test_seams_have_exactly_the_lengths():
    Q = GRAPHS["standin_g2"]
    form, target = lf.form_seams(Q, np.random.default_rng(6))
    want = np.where(target >= 0, target, np.diff(Q.indptr))
    check_form(Q, form, want)
    got = np.diff(form[0])
    for n in lf.SEAM_LENGTHS:
        assert (got == n).sum() >= 40


@pytest.mark.parametrize("name,n_hubs", [("hubs", 2), ("many_hubs", 200)])
@pytest.mark.parametrize("factor", [2, 3])
def test_hub_rows_cut(name, n_hubs, factor):
    Q = GRAPHS[name]
    deg = np.diff(Q.indptr)
    want = deg.copy()
    want[:n_hubs] *= factor
    check_form(Q, lf.form_rows(Q, np.arange(n_hubs), factor, np.random.default_rng(factor)), want)
    assert deg[:n_hubs].min() > deg[n_hubs:].max()                        # the hubs are the first vertices


@pytest.mark.parametrize("cls", lf.CLASS_NAMES)
def test_promotion_to_one_class(cls):
    Q = GRAPHS["standin_g1"]
    form, target = lf.form_promote(Q, cls, np.random.default_rng(8))
    indptr = check_form(Q, form, np.where(target >= 0, target, np.diff(Q.indptr)))
    assert (target >= 0).sum() == Q.shape[0] // 50
    assert lf.class_counts(indptr)[cls] >= Q.shape[0] // 50
    assert lf.class_counts(np.asarray([0, lf.PROMOTE_LENGTHS[cls]]))[cls] == 1


def test_class_and_pass_counts():
    indptr = np.concatenate([[0], np.cumsum([0, 1, 64, 65, 128, 129, 512, 513, 1024, 1025, 4096, 4097, 8192, 8193, 30000])])
    assert lf.class_counts(indptr) == {"le64": 3, "le128": 2, "mid1": 2, "midP": 4, "big": 4}
    assert lf.pass_counts(indptr) == ([1, 2, 3, 8], [1, 2, 4], [2, 3, 8])


def test_many_hubs_and_components_graphs():
    A, deg = lf.many_hubs_graph()
    got = np.diff(A.indptr)
    assert np.array_equal(got[:200], deg) and got[200:].max() < 130 and got[200:].min() >= 2
    assert deg.min() == 130 and deg.max() == 9000 and ((deg > 512) & (deg <= 4096)).sum() > 20 and (deg > 4096).sum() > 10
    B, comp = lf.components_graph()
    from scipy.sparse.csgraph import connected_components
    n, found = connected_components(B, directed=False)
    assert n == 302 + 50 and (np.diff(B.indptr)[comp < 0] == 0).all() and (comp < 0).sum() == 50
    pairs = np.unique(np.stack([found[comp >= 0], comp[comp >= 0]], axis=1), axis=0)
    assert len(pairs) == 302                                              # the planted components are the components
    assert sorted(np.bincount(comp[comp >= 0]).tolist())[-2:] == [3000, 3000]
