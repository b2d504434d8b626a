"""The contract of libgficf_sparse_query.so (include/gficf_sparse_query.h) restated in NumPy, rounding for rounding, and the
amplifier cases of its exact tests.

No new arithmetic: the header reuses the method of the square search word for word, so the contract table of (train, Q) is the
restatement of that search (tests/helpers/sparse_knn_par.py, unchanged) on the stacked matrix [train | Q], its query rows
[N, N + M) and its candidate columns [0, N).  The one thing the square contract adds, the diagonal written without arithmetic,
lands in the columns [N, N + M), which are cut away.

:func:`split` turns a case of tests/helpers/sparse_knn_cases.py into (train, Q): the training set is every column that is not the
SECOND member of an amplifier or manhattan pair; the queries are those second members, then a dozen long training cells repeated
(exact duplicates of training cells), then the empty cell, then, where M would be even, one more duplicate: M is a multiple of
no tile width above 1.  With one direction of a pair a query, every wrong order still changes 5 query -> twin distances or more at
every (metric, width) (tests/test_sparse_query_cpu.py prints the table): no second case with the roles exchanged is needed."""
import functools

import numpy as np
import scipy.sparse as sp

from tests.helpers import sparse_knn_cases as sc
from tests.helpers import sparse_knn_par as par
from tests.helpers import sparse_query_oracle as qo

METRICS, VARIANTS = par.METRICS, par.VARIANTS
N_DUPLICATES = 12


def distance_table(train, Q, metric, variant=None, variant_scope="all"):
    """The M x N f32 distances of every query to every training cell under the contract (or a wrong ``variant``)."""
    N, M = train.shape[1], Q.shape[1]
    return np.ascontiguousarray(par.distance_table(qo.stacked(train, Q), metric, N, N + M, variant, variant_scope)[:, :N])


def twin_distances(train, Q, metric, twins, variant=None, variant_scope="all"):
    """The f32 distances query -> twin of ``twins`` (n, 2): (position in Q, 0-based training id); entries of :func:`distance_table`."""
    N = train.shape[1]
    pairs = np.stack([twins[:, 0] + N, twins[:, 1]], axis=1)
    return np.ascontiguousarray(par.pair_distances(qo.stacked(train, Q), metric, pairs, variant, variant_scope)[:, 0])


table = par.table


@functools.lru_cache(maxsize=None)
def split(G):
    """{"train": G x N CSC, "Q": G x M CSC, "twins": (n, 2) (query position, training id) of the amplifier pairs, "mtwins": of the
    manhattan pairs, "duplicates": (n, 2) (query position, training id it repeats), "empty": the empty cell's query position}."""
    c = sc.case(G)
    A = c["M"]
    n_all, lengths = A.shape[1], np.diff(A.indptr)
    both = np.concatenate([c["pairs"], c["mpairs"]])
    out = both[:, 1]                                           # the columns that leave the training set
    assert len(set(out)) == len(out)
    keep = np.setdiff1d(np.arange(n_all), out)
    new_id = np.full(n_all, -1)
    new_id[keep] = np.arange(len(keep))
    in_pair = np.zeros(n_all, dtype=bool)
    in_pair[both.ravel()] = True
    free = np.flatnonzero(~in_pair)
    long_cells = free[np.argsort(-lengths[free], kind="stable")[:N_DUPLICATES]]
    empty = int(np.flatnonzero(lengths == 0)[0])
    q_cols = list(out) + list(long_cells) + [empty]
    if len(q_cols) % 2 == 0:
        q_cols.append(int(free[np.argsort(-lengths[free], kind="stable")[N_DUPLICATES]]))
    assert len(q_cols) % 2 == 1
    n_a = len(c["pairs"])
    twins = np.stack([np.arange(len(both)), new_id[both[:, 0]]], axis=1)
    assert (twins[:, 1] >= 0).all()
    dup_pos = np.arange(len(both), len(q_cols))
    duplicates = np.stack([dup_pos, new_id[np.array(q_cols)[dup_pos]]], axis=1)
    assert (duplicates[:, 1] >= 0).all()
    train, Q = sp.csc_matrix(A[:, keep]), sp.csc_matrix(A[:, q_cols])
    train.sort_indices()
    Q.sort_indices()
    return {"train": train, "Q": Q, "twins": twins[:n_a], "mtwins": twins[n_a:], "duplicates": duplicates,
            "empty": len(both) + len(long_cells)}


@functools.lru_cache(maxsize=None)
def contract(G, metric, variant=None):
    """The M x N f32 contract table of ``split(G)``; read-only."""
    s = split(G)
    d = distance_table(s["train"], s["Q"], metric, variant)
    d.setflags(write=False)
    return d
