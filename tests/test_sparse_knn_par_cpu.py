"""No GPU: the restatement of the sparse search's contract (tests/helpers/sparse_knn_par.py) and the inputs built for it
(tests/helpers/sparse_knn_cases.py).  The port agrees with the NumPy oracle under the oracle's rule; its chains and tree are a
scalar loop's; and three conditions on the INPUTS, none of them a measurement of the kernel: each deliberately wrong summation
order changes f32 bits of the amplifier pairs' distances at every tile width, it changes none between ordinary cells (which is why
the pairs are there), and the cases have the lengths, rows and placements the device tests rely on."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.helpers import sparse_knn_cases as sc
from tests.helpers import sparse_knn_oracle as so
from tests.helpers import sparse_knn_par as par

TQS = (8, 4, 2, 1)
MIN_CHANGED = 3


def _scalar_chain_sum(terms):
    """The header's words on 16 Python floats."""
    c = [0.0] * 16
    for e, t in enumerate(terms):
        c[e % 16] = c[e % 16] + float(t)
    for m in (8, 4, 2, 1):
        c = [c[l] + c[l ^ m] for l in range(16)]
    assert len(set(c)) == 1                                   # every lane ends with the sum
    return c[0]


@pytest.mark.parametrize("n", (0, 1, 15, 16, 17, 65))
def test_chains_and_tree_against_a_scalar_loop(n):
    rng = np.random.default_rng(n)
    terms = rng.gamma(2, 1, (3, n)) * 2.0 ** rng.uniform(-20, 20, (3, n)) * rng.choice([-1.0, 1.0], (3, n))
    got = par.chain_sum(terms)
    assert got.shape == (3,) and [float(g) for g in got] == [_scalar_chain_sum(t) for t in terms]
    if n == 65:                                               # the wrong orders are other sums
        assert all((par.chain_sum(terms, v) != got).any() for v in par.VARIANTS)


def _signed_case():
    rng = np.random.default_rng(4)
    M = so.case(60, 50, 0.3, 2)
    M.data *= rng.choice([-1.0, 1.0], M.nnz)
    M = sp.hstack([M, sp.csc_matrix((60, 1))], format="csc")   # and an empty cell
    M.sort_indices()
    return M


@pytest.mark.parametrize("metric", so.METRICS)
@pytest.mark.parametrize("which", ("signed", "oracle_case"))
def test_port_agrees_with_the_oracle(which, metric):
    M = _signed_case() if which == "signed" else so.case(30, 40, 0.3, 1)
    N = M.shape[1]
    d = par.distance_table(M, metric)
    if which == "signed" and metric in ("cosine", "correlation"):
        assert d.max() > 1                                    # a negative pair sum
    for k in (1, 10, N):
        idx, dist = par.table(d, k)
        want = so.oracle(M, metric, k)
        assert so.compare({"idx": idx, "dist": dist}, want, metric) == []
        assert np.array_equal(idx, want["idx"])
    a = 7                                                     # a query range is the rows of the table
    assert np.array_equal(np.concatenate([par.distance_table(M, metric, 0, a), par.distance_table(M, metric, a, N)]), d)
    pairs = np.array([[0, 1], [5, N - 1], [N - 2, 3]])
    assert np.array_equal(par.pair_distances(M, metric, pairs), np.stack([d[pairs[:, 0], pairs[:, 1]], d[pairs[:, 1], pairs[:, 0]]], axis=1))


@pytest.mark.parametrize("tq", TQS)
def test_the_cases_hold_what_the_device_tests_rely_on(tq):
    G = sc.tile_genes()[tq]
    c = sc.case(G)
    M = c["M"]
    N, lengths = M.shape[1], np.diff(M.indptr)
    assert N % 8 and N >= 129 and M.indices.min() == 0 and M.indices.max() == G - 1
    assert {min(n, G) for n in sc.LONG_LENGTHS} <= set(lengths) and (M.data < 0).any() and (lengths == 0).any()
    for pairs in (c["pairs"], c["mpairs"]):
        i, j = pairs[:, 0], pairs[:, 1]
        assert (lengths[i] >= 65).all() and (lengths[i] == lengths[j]).all()
        same_tile = i // tq == j // tq
        assert (~same_tile).sum() >= 10 and (tq == 1 or same_tile.sum() >= 10)
    a = c["split_at"]
    assert (a % tq or tq == 1) and ((c["pairs"][:, 0] == a - 1) & (c["pairs"][:, 1] == a)).any()


@pytest.mark.parametrize("metric", so.METRICS)
@pytest.mark.parametrize("tq", TQS)
def test_the_amplifier_discriminates(tq, metric):
    """Every wrong order, in every sum or in the pair sums alone, changes the f32 bits of at least MIN_CHANGED pairs."""
    G = sc.tile_genes()[tq]
    c = sc.case(G)
    pairs = c["mpairs"] if metric == "manhattan" else c["pairs"]
    want = sc.pair_bits(sc.contract(G, metric), pairs)
    assert np.array_equal(par.pair_distances(c["M"], metric, pairs).view(np.uint32), want)
    for scope in ("all", "pair"):
        for variant in par.VARIANTS:
            got = par.pair_distances(c["M"], metric, pairs, variant, scope).view(np.uint32)
            changed = int((got != want).any(axis=1).sum())
            print(f"TQ {tq} G {G} {metric} {variant} in {scope} sums: {changed} of {len(pairs)} pairs change")
            assert changed >= MIN_CHANGED, (variant, scope, changed)


@pytest.mark.parametrize("metric", so.METRICS)
@pytest.mark.parametrize("tq", TQS)
def test_ordinary_pairs_are_blind(tq, metric):
    """Between cells that are no pair, no wrong order changes one bit: without the amplifier the order is not observed."""
    G = sc.tile_genes()[tq]
    c = sc.case(G)
    want = sc.contract(G, metric).view(np.uint32)
    for variant in par.VARIANTS:
        got = par.distance_table(c["M"], metric, variant=variant).view(np.uint32)
        assert np.array_equal(got[c["ordinary"]], want[c["ordinary"]]), variant
