"""No GPU: the exact restatement of SLM's parallel form (tests/helpers/slm_par.py) — that the inputs of tests/test_slm_exact_gpu.py
qualify, and the properties include/gficf_slm.h states, on the restatement itself."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.helpers import closed_form, leiden_cases, leiden_par, slm_cases, slm_par


@pytest.mark.parametrize("name,seed", slm_cases.QUALIFIED)
def test_listed_pairs_qualify(name, seed):
    run = slm_cases.exact_run(name, seed)
    levels = max(r["level"] for r in run.trace) + 1
    print(name, seed, "fragile", run.fragile, "cap", run.exact_tie_cap, "levels of the deepest iteration", levels, "iterations", run.iterations)
    assert run.fragile == 0 and run.exact_tie_cap == 0
    assert (levels >= 3) == ((name, seed) in slm_cases.DEEP)


def test_enough_pairs_qualify():
    assert len(set(slm_cases.QUALIFIED)) >= 10 and len(set(slm_cases.DEEP)) >= 3 and set(slm_cases.DEEP) <= set(slm_cases.QUALIFIED)
    listed = [(n, s) for n in leiden_cases.EXACT_NAMES for s in leiden_cases.exact_seeds(n)]
    extra = [p for p in slm_cases.QUALIFIED if p not in listed]
    assert all(n.startswith("standin") and 0 <= s <= 9 for n, s in extra), extra


@pytest.mark.parametrize("c,m", leiden_cases.RINGS)
def test_rings_of_cliques(c, m):
    A, clique = leiden_cases.ring(c, m)
    run = slm_par.slm(A, 0.8, 1, 2, 0)
    assert run.n_clusters == c and len(set(zip(run.labels.tolist(), clique.tolist()))) == c
    assert abs(run.modularity - closed_form.ring_of_cliques_modularity(c, m, 0.8)) < 1e-12


def test_submove_stays_inside_the_fence():
    A, res = leiden_cases.exact_inputs()["standin7"]
    N = A.shape[0]
    for P in (slm_cases.three_communities(A), np.zeros(N, dtype=np.int32), np.arange(N, dtype=np.int32)):
        sub, n_sub, passes, fragile = slm_par.submove(A, P, res)
        assert fragile == 0 and n_sub == len(np.unique(sub)) and (sub <= np.arange(N)).all() and (sub[sub] == sub).all()
        pairs = set(zip(sub.tolist(), P.tolist()))
        assert len(pairs) == n_sub, "a sub-community crosses the fence"
        if len(np.unique(P)) == N:
            assert n_sub == N and passes == 1                  # every vertex is its own fence: nothing may move
        else:
            assert n_sub < N
        # a vertex with no same-community entry stays alone
        C = sp.csr_matrix(A)
        for v in range(N):
            nb = C.indices[C.indptr[v]:C.indptr[v + 1]]
            if not (P[nb[nb != v]] == P[v]).any():
                assert sub[v] == v and (sub == v).sum() == 1, v


def test_resume_equals_whole():
    for name, seed in (("knn_blobs", 0), ("standin9", 1234)):
        A, res = leiden_cases.exact_inputs()[name]
        one = slm_par.slm(A, res, 1, 1, seed)
        two = slm_cases.exact_run(name, seed)
        resumed = slm_par.slm(A, res, 1, 1, seed, init=one.labels)
        assert np.array_equal(resumed.labels, two.labels) and resumed.modularity == two.modularity


def test_starts_together_equal_starts_one_by_one():
    A, res = leiden_cases.exact_inputs()["knn_noise_alg2"]
    for seed in (0, 0xFFFFFFFE):                              # the second wraps: seeds 2^32 - 2, 2^32 - 1, 0
        singles = [slm_par.slm(A, res, 1, 2, (seed + s) & 0xFFFFFFFF) for s in range(3)]
        best = max(range(3), key=lambda s: (singles[s].modularity, -s))
        got = slm_par.slm(A, res, 3, 2, seed)
        assert got.start == best and np.array_equal(got.labels, singles[best].labels) and got.modularity == singles[best].modularity
        assert got.iterations == singles[best].iterations
    tie = slm_par.slm(leiden_cases.ring(8, 5)[0], 0.8, 3, 2, 0)
    assert tie.start == 0                                     # every start finds the cliques: the first one is returned


def test_early_stop_returns_what_all_iterations_would():
    for name, seed in (("planted8_res08", 0), ("knn_noise_alg2", 0)):
        A, res = leiden_cases.exact_inputs()[name]
        early = slm_par.slm(A, res, 1, 10, seed)
        full = slm_par.slm(A, res, 1, 10, seed, early_stop=False)
        assert early.iterations < 10 == full.iterations
        assert np.array_equal(early.labels, full.labels) and early.modularity == full.modularity


def test_the_restatement_leaves_leidens_alone():
    assert slm_par.local_moving is leiden_par.local_moving and slm_par.aggregate is leiden_par.aggregate and slm_par.canonical is leiden_par.canonical
