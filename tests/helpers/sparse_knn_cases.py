"""Inputs on which the contract of the sparse search (include/gficf_sparse_knn.h) shows, and the contract's tables of them
(tests/helpers/sparse_knn_par.py), computed once per process and shared by the CPU and the device tests.

:func:`case` builds one matrix from (G, seed); G sets the tile width (:func:`tile_genes` reads the G of every width off the
shape entry).  Its cells, in this order:

  * ``adjacent`` amplifier pairs, cell 2 i and its copy 2 i + 1: the same tile at every tile width above 1;
  * the first cells of the ``split`` amplifier pairs (their copies come after the long cells: another tile at every width);
  * the long cells: lengths cycling through :data:`LONG_LENGTHS` (the 4 x 16 unroll step of ``sk_chain`` +- 1, the 64-lane
    stride of the query scatter +- 1, the 701 entries of the measured workload, 1500), each capped at G, ``gamma(2, 1)``
    values, rows drawn from all of [0, G) with four fifths of the draws on a hot set of genes, so that two cells share
    genes at every G; rows 0 and G - 1 are both stored by the first of them;
  * the signed cells: negative values among the positive ones (``fabs``, a negative pair sum), one of them the negated, nudged
    copy of another (a cosine distance of 2), and one empty cell (the zero norm);
  * the copies of the split pairs;
  * the manhattan pairs, adjacent then split: values ``gamma * 2^U(-s, s)``, the copy with the smaller half of them moved by
    one f32 ulp each, up or down.

An amplifier pair is a cell and its copy with ONE value nudged by a relative 2^-10 ... 2^-22 (one f32 ulp at least).  The
distance of the two is then a cancellation: na + nb - 2 S is 10^-9 of its terms, so the roundings of the three f64 sums, 2^-53
of the terms, move the f32 bits of the result.  Between ordinary cells the same roundings sit 29 bits below the f32 rounding
and no order of summation shows.  Sums of f32 ``gamma`` values are exact in f64 (the exponents spread over a few bits, the sum
of a thousand 24-bit values fits 53 bits), so manhattan, whose terms are sums and differences alone, gets pairs of its own
with exponents spread over 2 s bits.  A copy with ONE value moved does not serve there: where a = b the term is 2 a exactly, so
T = 2 la bit for bit in every order, and la + lb - T does not see an order that la, lb and T share.  Moving the smaller half
of the values by an ulp each, in both directions, makes T a sum of its own (2 min(a, b)), and the distance, the sum of those
ulps, is small against the roundings of sums that the larger half dominates.  s = 20 keeps every value, square and sum far
inside f32 and f64; measured on the CPU at s = 6, 12, 20 and 300 or 1000 entries, 24 pairs: at s = 6 no wrong order changes a
bit, at s = 12 "lanes8" changes none, at s = 20 every wrong order changes 4 pairs or more."""
import functools

import numpy as np
import scipy.sparse as sp

from tests.helpers import sparse_knn_par as par

SEED = 11
LONG_LENGTHS = (47, 48, 49, 63, 64, 65, 79, 80, 81, 127, 128, 129, 255, 257, 701, 1500)
PAIR_LENGTHS = (65, 79, 81, 127, 129, 255, 257, 701, 1000)
N_LONG, N_PAIRS, N_MPAIRS, N_SIGNED = 60, 40, 24, 6
MANH_LENGTH, MANH_SPREAD = 1000, 20


def _rows(rng, G, n, hot):
    """n distinct rows of [0, G), ascending: four fifths of the weight on the hot genes."""
    p = np.full(G, 0.2 / G)
    p[hot] += 0.8 / len(hot)
    return np.sort(rng.choice(G, n, replace=False, p=p / p.sum()))


def _nudged(rng, v, j):
    """v with one value moved by a relative 2^-j in f32, one ulp at least."""
    w = v.astype(np.float32)
    at = int(rng.integers(len(w)))
    moved = np.float32(w[at] * np.float32(1.0 + 2.0 ** -j))
    if moved == w[at]:
        moved = np.nextafter(w[at], np.float32(np.inf))
    out = v.copy()
    out[at] = float(moved)
    return out


def _nudged_half(rng, v):
    """v with the smaller half of its values moved by one f32 ulp each, up or down."""
    w = v.astype(np.float32)
    small = np.argsort(np.abs(w), kind="stable")[:len(w) // 2]
    up = rng.random(len(small)) < 0.5
    w[small] = np.nextafter(w[small], np.where(up, np.float32(np.inf), np.float32(0.0)).astype(np.float32))
    return w.astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(G, seed=SEED):
    """{"M": genes x cells CSC (f64 values), "pairs": amplifier pairs (n, 2), "mpairs": manhattan's pairs (n, 2), "ordinary":
    N x N bool, True off the diagonal and off every pair, "split_at": a query id inside an adjacent pair, odd}."""
    rng = np.random.default_rng(seed)
    hot = rng.choice(G, min(G, 2000), replace=False)

    def cell(n):
        r = _rows(rng, G, min(n, G), hot)
        return r, rng.gamma(2, 1, len(r))

    amp, manh = [], []
    for i in range(N_PAIRS):
        r, v = cell(PAIR_LENGTHS[i % len(PAIR_LENGTHS)])
        amp.append(((r, v), (r, _nudged(rng, v, 10 + i % 13))))
    for i in range(N_MPAIRS):
        r, v = cell(MANH_LENGTH)
        v = v * 2.0 ** rng.uniform(-MANH_SPREAD, MANH_SPREAD, len(v))
        manh.append(((r, v), (r, _nudged_half(rng, v))))
    long_cells = [cell(LONG_LENGTHS[i % len(LONG_LENGTHS)]) for i in range(N_LONG)]
    r0, v0 = long_cells[0]
    r0 = np.unique(np.concatenate([[0, G - 1], r0[1:-1]]))    # rows 0 and G - 1 are stored somewhere
    long_cells[0] = (r0, v0[:len(r0)])
    signed = []
    for i in range(N_SIGNED - 2):
        r, v = cell(100 + i)
        signed.append((r, v * rng.choice([-1.0, 1.0], len(v))))
    signed.append((signed[0][0], _nudged(rng, -signed[0][1], 12)))
    signed.append((np.zeros(0, dtype=np.int64), np.zeros(0)))  # the empty cell

    cols, amp_ids, manh_ids = [], [], []

    def place(group, ids, adjacent):
        first = [len(cols) + (2 * i if adjacent else i) for i in range(len(group))]
        if adjacent:
            for a, b in group:
                cols.extend((a, b))
            ids.extend((f, f + 1) for f in first)
        else:
            cols.extend(a for a, _ in group)
        return first

    half, mhalf = N_PAIRS // 2, N_MPAIRS // 2
    place(amp[:half], amp_ids, True)
    split_first = place(amp[half:], amp_ids, False)
    cols.extend(long_cells)
    cols.extend(signed)
    amp_ids.extend((f, len(cols) + i) for i, f in enumerate(split_first))
    cols.extend(b for _, b in amp[half:])
    if len(cols) % 2:
        cols.append(cell(30))                                 # the adjacent manhattan pairs start at an even id
    place(manh[:mhalf], manh_ids, True)
    msplit_first = place(manh[mhalf:], manh_ids, False)
    cols.append(cell(30))
    manh_ids.extend((f, len(cols) + i) for i, f in enumerate(msplit_first))
    cols.extend(b for _, b in manh[mhalf:])
    if len(cols) % 8 == 0:
        cols.append(cell(30))                                 # N is no multiple of any tile width above 1

    N = len(cols)
    indptr = np.concatenate([[0], np.cumsum([len(r) for r, _ in cols])])
    M = sp.csc_matrix((np.concatenate([v for _, v in cols]), np.concatenate([r for r, _ in cols]).astype(np.int32), indptr), shape=(G, N))
    assert M.nnz == indptr[-1]
    pairs_a, mpairs_a = np.array(amp_ids), np.array(manh_ids)
    ordinary = ~np.eye(N, dtype=bool)
    for p in (pairs_a, mpairs_a):
        ordinary[p[:, 0], p[:, 1]] = ordinary[p[:, 1], p[:, 0]] = False
    split_at = int(pairs_a[6, 1])
    assert split_at % 2 == 1 and pairs_a[6, 0] == split_at - 1
    rows = M.indices
    assert rows.min() == 0 and rows.max() == G - 1 and N % 8 != 0 and N >= 129
    return {"M": M, "pairs": pairs_a, "mpairs": mpairs_a, "ordinary": ordinary, "split_at": split_at}


@functools.lru_cache(maxsize=None)
def tile_genes():
    """{TQ: the G of the case of that tile width}: 300 for the widest, else the first G the shape entry gives that width (one
    above the largest G of the next wider one, found as tests/test_sparse_knn_gpu.py's ``_seams`` finds it)."""
    import gficf_amd

    tq_of = lambda G: gficf_amd.find_nn_sparse_shape(G, 300, 16)["tile_queries"]
    top = gficf_amd.find_nn_sparse_shape(1, 300, 16)["max_genes"]
    out = {8: 300}
    for tq in (4, 2, 1):
        lo, hi = 1, top                                       # the largest G with tile_queries >= 2 tq
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if tq_of(mid) >= 2 * tq else (lo, mid - 1)
        out[tq] = lo + 1
    for tq, G in out.items():
        assert tq_of(G) == tq, (tq, G)
    return out


@functools.lru_cache(maxsize=None)
def contract(G, metric, variant=None):
    """The N x N f32 distance table of ``case(G)`` under the contract (or with every sum in a wrong ``variant``); read-only."""
    d = par.distance_table(case(G)["M"], metric, variant=variant)
    d.setflags(write=False)
    return d


def pair_bits(d, pairs):
    """The f32 bits of the mutual distances of ``pairs`` in the full table d: (n, 2) uint32, [i -> j, j -> i]."""
    return np.stack([d[pairs[:, 0], pairs[:, 1]], d[pairs[:, 1], pairs[:, 0]]], axis=1).view(np.uint32)
