"""GPU: the pruned kNN search (gficf_amd/csrc/knn.hip) where its cell layout and its bounds can go wrong — regimes that the
forced-prune cases of tests/test_knn_gpu.py (2 to 36 cells of 256 points) never reach.  The hooks: ``GFICF_KNN_PRUNE`` forces
the form, ``GFICF_KNN_PIVOT_CELL`` sets the points per pivot (so a few thousand points make thousands of cells) and
``GFICF_KNN_SPLIT`` the number of candidate slices of the plain form; the library reads them at call time.

Bar, as everywhere for the search: ``idx`` identical to ``oracle.knn`` (the same f32 chain, ties by index), ``dist`` equal as
f32.  The cell arithmetic quoted in the comments is ``knn_pivots`` / ``knn_coarse`` of knn.hip:
``C = clip(ceil(N / per), 2, 4096)`` fine pivots (rows ``r * (N // C)`` of the input), ``Cc = max(C // 16, 2)`` coarse ones
(every ``C // Cc``-th fine pivot); a point's sort key is ``(coarse - 1) << 12 | (fine - 1)``."""
import numpy as np
import pytest

import gficf_amd
import oracle
from oracle import oracle_np

pytestmark = pytest.mark.gpu

METRICS = ["manhattan", "euclidean", "cosine", "correlation"]


@pytest.fixture(scope="module")
def ops():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return gficf_amd.HipOps(0)


def blobs(N, d, seed, centers=12):
    """Clustered points (like cells in PCA space): Gaussian blobs with unequal spreads."""
    rng = np.random.default_rng(seed)
    c = rng.normal(scale=6.0, size=(centers, d))
    lab = rng.integers(0, centers, size=N)
    return c[lab] + rng.normal(size=(N, d)) * rng.uniform(0.5, 2.0, size=(centers, 1))[lab]


def n_pivots(N, per):
    """knn_pivots / knn_coarse of knn.hip."""
    C = min(max(-(-N // per), 2), 4096)
    return C, max(C // 16, 2)


_cache = {}


def cached(key, make):
    """One input / one oracle answer per key for the whole module; the arrays are handed out read-only."""
    if key not in _cache:
        val = make()
        for a in (val if isinstance(val, tuple) else (val,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = val
    return _cache[key]


def want(name, X, k, metric):
    return cached(("want", name, k, metric), lambda: oracle.knn(X, k, metric, nthreads=16))


def check_host(X, k, metric, widx, wdist, note=""):
    got = gficf_amd.find_nn(X, k, True, metric)
    assert got["idx"].shape == widx.shape and got["idx"].dtype == np.int32
    assert np.array_equal(got["idx"], widx), (metric, note)
    assert np.array_equal(got["dist"].astype(np.float32), wdist.astype(np.float32)), (metric, note)
    return got


def prepare(ops, X, metric):
    """Point rows of X on the device, as knn_search and knn_pivot_order take them."""
    import torch

    N, d = X.shape
    Xd = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()                     # (d, N) == column-major N x d
    pts = torch.zeros((N, ops.knn_dpad(d)), dtype=torch.float32, device="cuda")
    ops.knn_prepare(Xd, N, d, metric, pts)
    return pts


def search_block(ops, pts, N, d, k, metric, b, e):
    """Queries [b, e) through the device entry into sentinel-filled outputs -> (idx, dist) as (e - b) x k."""
    import torch

    ws = torch.zeros(ops.knn_workspace_bytes(e - b, N, k), dtype=torch.uint8, device="cuda")
    idx = torch.full((k, e - b), -7, dtype=torch.int32, device="cuda")
    dist = torch.full((k, e - b), -7.0, dtype=torch.float32, device="cuda")
    ops.knn_search(pts, N, d, k, metric, b, e, ws, idx, dist)
    ops.sync()
    return idx.cpu().numpy().T, dist.cpu().numpy().T


# ------------------------------------------------------------------------------------------- A. many, tiny and empty cells
# N, d, k, per                                   C = clip(ceil(N / per), 2, 4096), Cc = max(C // 16, 2)
MANY_CELLS = [
    (5000, 10, 15, 4),     # C = 1250, Cc = 78: k_knn_cell_offsets (1024 threads) takes ceil(1250 / 1024) = 2 cells per thread
    (9000, 6, 31, 3),      # C = 3000, Cc = 187: 3 cells per thread; the full 32-entry register list is not reached, 31 is
    (17000, 8, 10, 4),     # ceil(17000 / 4) = 4250 -> C capped at 4096, Cc = 256: fine keys up to 4095 (all 12 bits), coarse up to 255
                           # (all 20 bits of the cell sort), 4 cells per thread; 133 + 4096 candidate and 266 + 4096 query tiles at most
    (3000, 5, 65, 2),      # C = 1500, Cc = 93: lists in LDS (k > 64), every cell (~2 points) far smaller than k
]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("N,d,k,per", MANY_CELLS)
def test_thousands_of_tiny_cells(N, d, k, per, metric, monkeypatch):
    """Cells of 1 to a few points: every one pads to a 128-row candidate tile and a 64-row query tile that are almost all padding."""
    C, Cc = n_pivots(N, per)
    assert C > 1024 and (C == 4096) == (N == 17000) and (Cc == 256) == (N == 17000)
    X = cached(("blobs", N, d), lambda: blobs(N, d, seed=N + d + k))
    widx, wdist = want(("blobs", N, d), X, k, metric)
    monkeypatch.setenv("GFICF_KNN_PRUNE", "1")
    monkeypatch.setenv("GFICF_KNN_PIVOT_CELL", str(per))
    check_host(X, k, metric, widx, wdist)


def _few_points_repeated(shuffled):
    rng = np.random.default_rng(40)
    X = np.repeat(rng.normal(scale=4.0, size=(40, 3)), 60, axis=0)          # 40 distinct points, 60 copies each: N = 2400
    return X[rng.permutation(len(X))] if shuffled else X


@pytest.mark.parametrize("metric", ["manhattan", "euclidean"])
@pytest.mark.parametrize("shuffled", [False, True])
def test_empty_cells_from_coinciding_pivots(shuffled, metric, monkeypatch):
    """N = 2400, per = 8: C = 300 pivots (rows r * 8) drawn from 40 distinct points, so most pivots coincide with an earlier one; the
    nearest-pivot search gives all their points to the smallest index and the others own no cell (no key, no tile)."""
    X = cached(("repeated", shuffled), lambda: _few_points_repeated(shuffled))
    N, k, per = len(X), 17, 8
    C, _ = n_pivots(N, per)
    assert C == 300
    pivots = X[np.arange(C) * (N // C)]
    assert len(np.unique(pivots, axis=0)) <= C - 2, "premise: at least two pivot rows coincide, so an empty cell exists"
    widx, wdist = want(("repeated", shuffled), X, k, metric)
    monkeypatch.setenv("GFICF_KNN_PRUNE", "1")
    monkeypatch.setenv("GFICF_KNN_PIVOT_CELL", str(per))
    check_host(X, k, metric, widx, wdist)
    assert np.all(wdist[:, :k] == 0.0)                                          # 60 copies each: the 17 nearest are copies


@pytest.mark.parametrize("metric", ["manhattan", "cosine"])
def test_query_blocks_over_tiny_cells(ops, metric, monkeypatch):
    """The device entry with query blocks of 1, 64, 2935 and 2000 rows over N = 5000, per = 4 (C = 1250, Cc = 78): the query layout
    is built per block (a block of one query is one cell in one tile), the candidate layout is the same every time."""
    N, d, k, per = 5000, 10, 15, 4
    assert n_pivots(N, per) == (1250, 78)
    X = cached(("blobs", N, d), lambda: blobs(N, d, seed=N + d + k))
    widx, wdist = want(("blobs", N, d), X, k, metric)
    monkeypatch.setenv("GFICF_KNN_PRUNE", "1")
    monkeypatch.setenv("GFICF_KNN_PIVOT_CELL", str(per))
    pts = prepare(ops, X, metric)
    out = [search_block(ops, pts, N, d, k, metric, b, e) for b, e in ((0, 1), (1, 65), (65, 3000), (3000, 5000))]
    idx, dist = np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])
    assert not np.any(idx == -7) and not np.any(dist == -7.0)
    assert np.array_equal(idx, widx)
    assert np.array_equal(dist, wdist.astype(np.float32))


# --------------------------------------------------------------- B. cosine / correlation keys below zero, zero rows
DUP_SEED = 0                 # recorded: with this draw 900-odd (k = 17) and 700-odd (k = 40) queries have a k-th distance below zero
DUP_ZERO_AT = np.array([0, 333, 401, 777, 1204])


def _repeated_directions(metric, permuted):
    """3 directions in 12-D, 400 copies each with magnitudes in (0.1, 10): after the f32 normalisation the copies are unit vectors
    an ulp or two apart, so many dots round above 1 and the keys 1 - dot below 0.  Five rows that normalise to nothing: all zero
    (cosine), constant 2.0 (correlation: 12 * 2.0 sums exactly, the mean is 2.0 and the centred row is zero)."""
    rng = np.random.default_rng(DUP_SEED)
    D = np.repeat(rng.normal(size=(3, 12)), 400, axis=0) * rng.uniform(0.1, 10.0, size=(1200, 1))
    X = np.empty((1205, 12))
    X[np.setdiff1d(np.arange(1205), DUP_ZERO_AT)] = D
    X[DUP_ZERO_AT] = 0.0 if metric == "cosine" else 2.0
    if not permuted:
        return X, DUP_ZERO_AT
    perm = np.random.default_rng(DUP_SEED + 1).permutation(1205)
    return X[perm], np.flatnonzero(np.isin(perm, DUP_ZERO_AT))


@pytest.mark.parametrize("form", ["plain", "pruned", "pruned-32"])
@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("k", [17, 40])
@pytest.mark.parametrize("metric", ["cosine", "correlation"])
def test_keys_below_zero_and_zero_rows(metric, k, permuted, form, monkeypatch):
    """The pruned traversal ends at the first tile whose bound exceeds the largest k-th best of the tile's queries, and the bound is
    clamped at 0: with k-th bests BELOW zero it must still reach every tile that holds a key at or below them.  (It does: the
    maximum the waves publish starts from 0, so a tile with bound 0 is always visited, and a tile with a positive bound holds
    positive keys only.)  N = 1205: 10 candidate tiles; default cells: C = 5 of ~241 points; per = 32: C = 38, a direction's 400
    copies span a dozen cells and tiles."""
    X, zero_at = cached(("dirs", metric, permuted), lambda: _repeated_directions(metric, permuted))
    widx, wdist = want(("dirs", metric, permuted), X, k, metric)
    # premises, from the input and the oracle alone
    assert (wdist[:, k - 1] < 0).any(), "premise: some query's k-th distance is below zero"
    assert np.all(wdist[zero_at] == 1.0), "premise: a row without direction is at distance exactly 1 from everything"
    assert np.array_equal(widx[zero_at], np.tile(np.arange(1, k + 1, dtype=np.int32), (5, 1)))      # all ties: the k smallest ids
    monkeypatch.setenv("GFICF_KNN_PRUNE", "0" if form == "plain" else "1")
    if form == "pruned-32":
        assert n_pivots(len(X), 32) == (38, 2)
        monkeypatch.setenv("GFICF_KNN_PIVOT_CELL", "32")
    got = check_host(X, k, metric, widx, wdist, form)
    assert np.all(got["dist"][zero_at] == 1.0)
    assert np.all(got["dist"][:, :k][got["idx"] == zero_at[0] + 1] == 1.0)      # ... and whoever lists such a row has it at exactly 1


# --------------------------------------------------------------------------------------- C. split seams for every metric
def _split_case(ops, N, d, metric):
    X = cached(("blobs", N, d), lambda: blobs(N, d, seed=N + d))
    return X, cached(("pts", N, d, metric), lambda: prepare(ops, X, metric))


@pytest.mark.parametrize("split", [1, 2, 5, 16])
@pytest.mark.parametrize("k", [31, 100])
@pytest.mark.parametrize("metric", METRICS)
def test_split_seams(ops, metric, k, split, monkeypatch):
    """The plain form with its 24 candidate tiles (N = 3000) cut into 1, 2, 5 and 16 slices, register lists (k = 31) and LDS lists
    (k = 100): the merge of the slices' lists (with its sqrtf for euclidean) gives the oracle's table.  d = 17: one full 16-dim
    chunk and a chunk of one dim.  Correlation is the cosine search on rows that knn_prepare centred."""
    N, d = 3000, 17
    X, pts = _split_case(ops, N, d, metric)
    widx, wdist = want(("blobs", N, d), X, k, metric)
    monkeypatch.setenv("GFICF_KNN_SPLIT", str(split))
    idx, dist = search_block(ops, pts, N, d, k, metric, 0, N)
    assert np.array_equal(idx, widx)
    assert np.array_equal(dist, wdist.astype(np.float32))


@pytest.mark.parametrize("N,k", [(300, 5), (300, 128), (128, 128)])
@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_slices_without_a_tile(ops, metric, N, k, monkeypatch):
    """16 slices over 3 candidate tiles (N = 300) or 1 (N = 128): slice sp covers tiles [n_ct * sp / 16, n_ct * (sp + 1) / 16), so 13
    (15) slices are empty and hand the merge a list of all-ones keys.  k = 128 is the library's longest list (GFICF_KNN_MAX_K);
    with N = 128 every point is a neighbour of every query."""
    d = 7
    X, pts = _split_case(ops, N, d, metric)
    widx, wdist = want(("blobs", N, d), X, k, metric)
    monkeypatch.setenv("GFICF_KNN_SPLIT", "16")
    idx, dist = search_block(ops, pts, N, d, k, metric, 0, N)
    assert np.array_equal(idx, widx)
    assert np.array_equal(dist, wdist.astype(np.float32))
    if k == N:
        assert np.array_equal(np.sort(idx, axis=1), np.tile(np.arange(1, N + 1, dtype=np.int32), (N, 1)))


def test_more_neighbours_than_the_longest_list_is_refused(ops, monkeypatch):
    """k = 300 of N = 300 points is beyond GFICF_KNN_MAX_K = 128: refused with its status before anything is launched, whatever the split."""
    import torch

    monkeypatch.setenv("GFICF_KNN_SPLIT", "16")
    X, pts = _split_case(ops, 300, 7, "euclidean")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    idx = torch.full((300, 300), -7, dtype=torch.int32, device="cuda")
    with pytest.raises(gficf_amd.GficfError) as ei:
        ops.knn_search(pts, 300, 7, 300, "euclidean", 0, 300, ws, idx, None)
    assert ei.value.status == "GFICF_ERR_UNSUPPORTED"
    ops.sync()
    assert bool((idx == -7).all())


# ------------------------------------------------------------------------------------- D. dimension and list-length seams
@pytest.mark.parametrize("prune", ["0", "1"])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [4, 15, 16, 17, 31, 32, 33, 127])
def test_dimension_seams(d, metric, prune, monkeypatch):
    """Around the 16-dim LDS chunk (15, 16, 17, 31, 32, 33: a last chunk of 15, 16 and 1 dims), one float4 per row (4) and the odd d
    under the cap (127: dpad = 128, the last pair of dims is one real and one padded)."""
    N, k = 700, 9
    X = cached(("blobs", N, d), lambda: blobs(N, d, seed=N + d + k))
    widx, wdist = want(("blobs", N, d), X, k, metric)
    monkeypatch.setenv("GFICF_KNN_PRUNE", prune)
    check_host(X, k, metric, widx, wdist)


@pytest.mark.parametrize("prune", ["0", "1"])
@pytest.mark.parametrize("metric", ["manhattan", "cosine"])
@pytest.mark.parametrize("k", [32, 34, 48, 63, 66, 127])
def test_list_length_seams(k, metric, prune, monkeypatch):
    """32: a full 32-entry register list (2 entries per lane).  34, 48, 63: the 64-entry list (4 per lane), whose k-th entry is
    entry (k - 1) % 4 = 1, 3, 2 of its lane — 34 is the one residue the other tests (33, 51, 64: 0, 2, 3) leave out.  66, 127: LDS lists."""
    N, d = 1100, 20
    X = cached(("blobs", N, d), lambda: blobs(N, d, seed=N + d))
    widx, wdist = want(("blobs", N, d), X, k, metric)
    monkeypatch.setenv("GFICF_KNN_PRUNE", prune)
    check_host(X, k, metric, widx, wdist)


@pytest.mark.parametrize("metric", ["manhattan", "euclidean", "cosine"])
def test_tiny_cells_against_float64_restatement(metric, monkeypatch):
    """The many-cell layout once against the independent float64 writing, with the tolerances of test_against_float64_restatement."""
    monkeypatch.setenv("GFICF_KNN_PRUNE", "1")
    monkeypatch.setenv("GFICF_KNN_PIVOT_CELL", "1")                            # N = 1500: C = 1500, every point a pivot, 2 cells per thread
    X = cached(("blobs", 1500, 12), lambda: blobs(1500, 12, seed=6))
    got = gficf_amd.find_nn(X, 20, True, metric)
    nidx, ndist = cached(("np", metric), lambda: oracle_np.knn_np(X, 20, metric))
    assert np.allclose(got["dist"], ndist, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------- E. knn_pivot_order by its definition
def pivot_order(ops, X, metric):
    import torch

    N, d = X.shape
    pts = prepare(ops, X, metric)
    ws = torch.zeros(ops.knn_workspace_bytes(N, N, 1), dtype=torch.uint8, device="cuda")
    order = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    ops.knn_pivot_order(pts, N, d, metric, ws, order)
    ops.sync()
    return order.cpu().numpy()


@pytest.mark.parametrize("metric", METRICS)
def test_pivot_order_is_a_permutation_and_repeats(ops, metric):
    X = cached(("blobs", 20000, 10), lambda: blobs(20000, 10, seed=31))       # C = 79, Cc = 4
    a = pivot_order(ops, X, metric)
    assert a.dtype == np.int32 and np.array_equal(np.sort(a), np.arange(20000, dtype=np.int32))
    assert np.array_equal(pivot_order(ops, X, metric), a)


GROUPS, PER_GROUP = 64, 300
MARGIN = 1e-3                # relative; f32 rounding of a 6-term sum of exact differences is below 1e-6


def _dists(A, B, metric):
    df = A[:, None, :] - B[None, :, :]
    return np.abs(df).sum(axis=2) if metric == "manhattan" else np.sqrt((df * df).sum(axis=2))


def _nearest(A, B, metric):
    """(index of the nearest row of B for every row of A — the smaller index on an exact tie, as the search does —, smallest relative
    margin by which a row of B that is not a copy of the nearest one is farther)."""
    D = _dists(A, B, metric)
    near = D.argmin(axis=1)
    dn = D[np.arange(len(A)), near]
    other = np.where((B[None, :, :] == B[near][:, None, :]).all(axis=2), np.inf, D)      # copies of the nearest pivot tie exactly
    return near, (other.min(axis=1) - dn) / other.min(axis=1)


def _far_apart_groups():
    """64 groups of 300 points in 6-D, the centres at least 100 apart (both metrics), the points within 0.5 of their centre (|offset|
    <= 0.08 per coordinate), values rounded to f32 (so the device sees the same numbers: no rounding of the 600-sized coordinates enters
    the 0.5-sized distances).  The order is shuffled, except that the C = 75 pivot rows r * 256 are filled so that every group owns a pivot (rows 0 .. 63 * 256:
    one group each, in random order; the other 11 from random groups) — a group without a pivot would have to choose between pivots
    100 away by a margin its own spread decides.  Points that sit within MARGIN of the bisector of two pivots of their group are
    drawn again, and the whole draw is repeated with the next seed while a fine pivot sits that close to the bisector of two coarse
    ones; what the test relies on is asserted by the test, not here."""
    for seed in range(64, 96):                                  # the first draw whose pivots all have an unambiguous coarse pivot
        X, group, centres, coarse_margin = _far_apart_groups_draw(seed)
        if coarse_margin >= 2 * MARGIN:
            break
    return X, group, centres


def _far_apart_groups_draw(seed):
    rng = np.random.default_rng(seed)
    N, d = GROUPS * PER_GROUP, 6
    C, Cc = n_pivots(N, 256)
    assert (C, Cc, N // C, C // Cc) == (75, 4, 256, 18)
    centres = np.empty((0, d))
    while len(centres) < GROUPS:
        c = rng.uniform(0.0, 600.0, size=d)
        if len(centres) == 0 or np.sqrt(((centres - c) ** 2).sum(axis=1)).min() >= 100.0:      # euclidean <= manhattan
            centres = np.vstack([centres, c])
    group = np.repeat(np.arange(GROUPS), PER_GROUP)
    pos = rng.permutation(N)                                    # pos[p] = point at row p
    prow = np.arange(C) * (N // C)
    pgroup = np.concatenate([rng.permutation(GROUPS), rng.integers(0, GROUPS, size=C - GROUPS)])
    for r, g in zip(prow, pgroup):                              # bring a point of group g to pivot row r (swap with a non-pivot row)
        if group[pos[r]] != g:
            cand = np.flatnonzero((group[pos] == g) & ~np.isin(np.arange(N), prow))
            pos[[r, cand[0]]] = pos[[cand[0], r]]
    group = group[pos]
    draw = lambda n: rng.uniform(-0.08, 0.08, size=(n, d))
    X = (centres[group] + draw(N)).astype(np.float32).astype(np.float64)
    fine = X[prow]                                              # (pivot rows are never drawn again)
    coarse_margin = min(_nearest(fine, fine[np.arange(Cc) * (C // Cc)], metric)[1].min() for metric in ("manhattan", "euclidean"))
    movable = ~np.isin(np.arange(N), prow)
    for _ in range(20 if coarse_margin >= 2 * MARGIN else 0):
        close = np.zeros(N, dtype=bool)
        for metric in ("manhattan", "euclidean"):
            close |= _nearest(X, X[prow], metric)[1] < 2 * MARGIN
        close &= movable
        if not close.any():
            break
        X[close] = (centres[group[close]] + draw(int(close.sum()))).astype(np.float32).astype(np.float64)
    return X, group, centres, coarse_margin


@pytest.mark.parametrize("metric", ["manhattan", "euclidean"])
def test_pivot_order_against_its_definition(ops, metric):
    """order = the points sorted (stably) by ((coarse pivot of their fine pivot) << 12 | fine pivot), the fine pivot being the nearest of
    the rows r * (N // C), the coarse pivot the nearest of every (C // Cc)-th fine pivot — all of it restated in numpy f64 on an input
    where every "nearest" is decided by a margin far above f32 rounding, so the expected order is the only right answer."""
    X, group, centres = cached("groups", _far_apart_groups)
    N = len(X)
    C, Cc = n_pivots(N, 256)
    # premises of the construction
    cd = _dists(centres, centres, "euclidean")
    assert cd[~np.eye(GROUPS, dtype=bool)].min() >= 100.0
    assert _dists(X, centres, "manhattan")[np.arange(N), group].max() <= 0.5
    assert np.array_equal(X, X.astype(np.float32).astype(np.float64))
    fine = X[np.arange(C) * (N // C)]
    coarse = fine[np.arange(Cc) * (C // Cc)]
    fine_of, m_fine = _nearest(X, fine, metric)
    coarse_of, m_coarse = _nearest(fine, coarse, metric)
    assert m_fine.min() >= MARGIN and m_coarse.min() >= MARGIN, "premise: every nearest pivot is unambiguous"
    assert len(np.unique(fine_of)) == C                         # 75 cells, none empty
    key = (coarse_of[fine_of].astype(np.int64) << 12) | fine_of
    expected = np.argsort(key, kind="stable").astype(np.int32)
    assert np.array_equal(pivot_order(ops, X, metric), expected)
