"""No GPU: the exact restatement of Leiden's parallel form (tests/helpers/leiden_par.py), the yardstick of
tests/test_leiden_exact_gpu.py, against the older yardsticks — connectivity, resumption, the reference partitions, the sequential
restatement's Q (tests/helpers/leiden_np.py) — and the QUALIFICATION of every input of the exact GPU tests: the restatement counts no
fragile decision on it (a decision the device's f64 evaluation may legitimately take the other way; leiden_par's docstring has the
thresholds), at every seed and resolution those tests use.  An input that does not qualify gets another generator seed, never another
threshold."""
import numpy as np
import pytest

from tests.helpers import closed_form, leiden_cases, leiden_np, leiden_par
from tests.helpers import louvain_forms as lf

GOLDEN = ["knn_blobs", "knn_noise_alg2", "planted3", "planted8_res08"]
RING_NAMES = [f"ring{c}x{m}" for c, m in leiden_cases.RINGS]
Q_TOL = 0.01                    # tests/test_leiden_gpu.py


def test_hash_is_the_header_s():
    # lowbias32 as include/gficf_leiden.h writes it out, evaluated by hand for 1: 1 * 0x7feb352d = 0x7feb352d; ^= >> 15 -> 0x7feb_caf9 ...
    v = 1
    v ^= v >> 16; v = v * 0x7feb352d % 2 ** 32; v ^= v >> 15; v = v * 0x846ca68b % 2 ** 32; v ^= v >> 16
    assert leiden_par.hash32(1) == v and leiden_par.hash32(0) == 0 and leiden_par.hash32(2 ** 32 + 1) == v
    assert leiden_par.level_seed(0, 0) == leiden_par.hash32(0x165667B1)
    assert leiden_par.level_seed(3, 2) == leiden_par.hash32((3 * 0x9E3779B1 + 2 * 0x85EBCA77 + 0x165667B1) % 2 ** 32)
    classes = np.bincount([leiden_par.hash32(v ^ leiden_par.level_seed(0, 0)) % 4 for v in range(4000)], minlength=4)
    assert classes.min() > 900                                      # four classes of about a quarter each


@pytest.mark.parametrize("name", leiden_cases.EXACT_NAMES)
def test_every_input_of_the_exact_tests_qualifies(name):
    A, res = leiden_cases.exact_inputs()[name]
    for seed in leiden_cases.exact_seeds(name):
        run = leiden_cases.exact_run(name, seed)
        print(name, "seed", seed, "fragile", run.fragile, "clusters", run.n_clusters, "Q", run.modularity,
              "passes", [t["passes"] for t in run.trace])
        assert run.fragile == 0 and run.exact_tie_cap == 0, (name, seed, run.fragile)
        assert max(t["passes"] for t in run.trace) < leiden_par.MAX_PASSES
        assert len(run.after) == 2 and run.levels[1] == len(run.trace)


def test_the_counter_reports_an_input_that_does_not_qualify():
    """knn_noise_alg2 at seed 1: level 2 of the first iteration oscillates to the pass cap with dQ exactly 0."""
    A, res, _ = leiden_cases.golden()["knn_noise_alg2"]
    run = leiden_par.leiden(A, res, 1, 1)
    print("fragile", run.fragile, "levels at the cap on an exact tie", run.exact_tie_cap, "passes", [t["passes"] for t in run.trace])
    assert run.fragile > 0 and run.exact_tie_cap == 1 and max(t["passes"] for t in run.trace) == leiden_par.MAX_PASSES
    # a comparison within 2^-40 of its terms is counted, one outside is not, identical operands never are
    P = leiden_par.Problem(A, res)
    assert P.close(1, 2 ** 40, False) and not P.close(1, 2 ** 40 - 1, False) and not P.close(0, 2 ** 40, True) and not P.close(0, 0, False)
    assert P.close(0, 5, False) and P.fragile == 2


@pytest.mark.parametrize("name", GOLDEN + RING_NAMES)
def test_against_the_older_yardsticks(name):
    A, res = leiden_cases.exact_inputs()[name]
    two = leiden_cases.exact_run(name, 0)
    one = two.after[0]
    fixed = A.copy()
    fixed.data = np.rint(A.data * lf.SCALE) / lf.SCALE                  # the graph the sums are taken over: 2^-32 fixed point
    for lab, nc, q in two.after:
        assert lab.dtype == np.int32 and lab.min() == 0 and lab.max() == nc - 1 and (np.diff(np.bincount(lab)) <= 0).all()
        assert leiden_np.communities_connected(A, lab)
        assert abs(q - leiden_np.modularity(fixed, lab, res)) < 1e-12
        assert abs(q - leiden_np.modularity(A, lab, res)) < 1e-9        # tests/test_leiden_gpu.py: check_labels
    # resumption: two iterations == one iteration resumed from its own result, trace included
    resumed = leiden_par.leiden(A, res, 1, 0, init=one[0])
    assert np.array_equal(resumed.labels, two.labels) and resumed.modularity == two.modularity and resumed.n_clusters == two.n_clusters
    assert resumed.trace == two.trace[two.levels[0]:]
    q_np = leiden_np.modularity(A, leiden_np.leiden(A, res, 2), res)
    print(name, "Q", two.modularity, "sequential restatement", q_np)
    assert abs(two.modularity - q_np) < Q_TOL
    if name in GOLDEN:
        if name != "knn_noise_alg2":
            assert leiden_np.same_partition(two.labels, leiden_cases.golden()[name][2])
    else:
        c, m = leiden_cases.RINGS[RING_NAMES.index(name)]
        assert two.n_clusters == c and leiden_np.same_partition(two.labels, leiden_cases.ring(c, m)[1])
        assert abs(two.modularity - closed_form.ring_of_cliques_modularity(c, m, 0.8)) < 1e-12


def test_the_figures_the_device_is_recorded_with():
    """DESIGN.md §15 records the device's Q on knn_noise_alg2 as 0.6535 where the sequential restatement has 0.6575: the exact
    restatement gives the device's figure, not the sequential one's."""
    q = leiden_cases.exact_run("knn_noise_alg2", 0).modularity
    assert abs(q - 0.653531) < 5e-7


def test_the_stages_alone():
    A, res = leiden_cases.exact_inputs()["knn_noise_alg2"]
    N = A.shape[0]
    lab, passes, q, fragile = leiden_par.move(A, np.arange(N), res)
    first = leiden_cases.exact_run("knn_noise_alg2", 0).trace[0]
    assert passes == first["passes"] and q == first["q"] and len(np.unique(lab)) == first["communities"] and fragile == 0
    R, n_ref, rounds, fragile = leiden_par.refine(A, lab, res)
    assert n_ref == first["refined"] and rounds == first["rounds"] and fragile == 0 and len(np.unique(R)) == n_ref
    assert np.array_equal(R, leiden_np.canonical(R)) and leiden_np.communities_connected(A, R)
    assert len(np.unique(np.stack([R, lab], axis=1), axis=0)) == n_ref               # every refined community inside one community
    assert leiden_np.refine_leftover(A, lab, R, res, 1e-6) == 0
    # the two-component community of the ring is split into its cliques
    A, clique, init = leiden_cases.disconnected_start(8, 5)
    R, n_ref, _, fragile = leiden_par.refine(A, init, 0.8)
    assert n_ref == 8 and fragile == 0 and leiden_np.same_partition(R, clique)


@pytest.mark.parametrize("name,start", [("knn_noise_alg2", "one community"), ("knn_blobs", "one community"), ("standin7", "one community"),
                                        ("standin7", "one iteration"), ("ring8x5", "two components"), ("ring60x10", "two components")])
def test_the_refinement_starts_that_need_no_device_qualify(name, start):
    A, res = leiden_cases.exact_inputs()[name]
    if start == "one community":
        P = np.zeros(A.shape[0], dtype=np.int32)
    elif start == "one iteration":
        P = leiden_cases.exact_run(name, 0).after[0][0]
    else:
        P = leiden_cases.disconnected_start(*leiden_cases.RINGS[RING_NAMES.index(name)])[2]
    R, n_ref, rounds, fragile = leiden_par.refine(A, P, res)
    print(name, start, "refined communities", n_ref, "rounds", rounds, "fragile", fragile)
    assert fragile == 0 and 1 < n_ref < A.shape[0] and leiden_np.refine_leftover(A, P, R, res, 1e-6) == 0


def test_forms_are_the_graph_and_give_its_labels():
    name = leiden_cases.PATH_GRAPH
    A, res = leiden_cases.exact_inputs()[name]
    N = A.shape[0]
    want = leiden_cases.exact_run(name, 0)
    canon = lf.fixed_point_matrix(*lf.canonical(A), N)
    seam, target = leiden_cases.seam_form(A, np.random.default_rng(5))
    forms = {"seams": seam, "all long": leiden_cases.all_long_form(A, np.random.default_rng(6)), "shuffled": lf.form_shuffle(A, np.random.default_rng(7))}
    assert np.array_equal(np.diff(seam[0]), np.where(target >= 0, target, np.diff(A.indptr)))
    assert leiden_cases.ld_path_counts(seam[0], N) == {"wave": N - 4 * leiden_cases.SEAM_ROWS, 1: 2 * leiden_cases.SEAM_ROWS,
                                                       2: leiden_cases.SEAM_ROWS, 3: leiden_cases.SEAM_ROWS}
    assert leiden_cases.ld_path_counts(forms["all long"][0], N) == {"wave": 0, 1: N}
    assert not np.array_equal(forms["shuffled"][1], A.indices) and np.array_equal(forms["shuffled"][0], A.indptr)
    for what, form in forms.items():
        assert (form[2] > 0).all() and lf.same_graph(lf.fixed_point_matrix(*form, N), canon), what
        got = leiden_par.leiden(form, res, 2, 0)
        assert got.fragile == 0 and np.array_equal(got.labels, want.labels) and got.modularity == want.modularity and got.trace == want.trace, what


@pytest.mark.parametrize("name", [f"small{s}" for s in leiden_cases.ZERO_SEEDS])
def test_stored_zeros_and_the_diagonal_are_no_edges(name):
    """The header's rule: a stored zero is no edge and the diagonal is ignored, so neither may carry a stamp.  The restatement gives
    the plain matrix's answer for both variants — and would NOT under the rule the header excludes (a mover stamps the target of every
    stored entry), on these very inputs: that is what tests/test_leiden_exact_gpu.py::test_stored_zeros_and_diagonal can see."""
    A, res = leiden_cases.exact_inputs()[name]
    want = leiden_cases.exact_run(name, 0)
    variants = {"zeros": leiden_cases.with_stored_zeros(A), "diagonal": leiden_cases.with_diagonal(A)}
    same_plain = leiden_par.leiden(A, res, 2, 0, stamp_stored=True)
    assert np.array_equal(same_plain.labels, want.labels) and same_plain.trace == want.trace     # without zeros the two rules are one
    for what, B in variants.items():
        got = leiden_par.leiden(B, res, 2, 0)
        assert got.fragile == 0 and np.array_equal(got.labels, want.labels) and got.modularity == want.modularity and got.trace == want.trace
        other = leiden_par.leiden(B, res, 2, 0, stamp_stored=True)
        assert other.fragile == 0 and not np.array_equal(other.labels, want.labels), (name, what)
