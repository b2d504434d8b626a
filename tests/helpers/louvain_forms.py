"""Forms of one graph for the Louvain kernels (tests/test_louvain_paths_gpu.py, tests/test_louvain_forms_cpu.py).

gficf_amd/csrc/louvain.hip sums weights as integers in 2^-32 fixed point and picks a row's kernel by the row's LENGTH (stored entries,
not distinct neighbours).  So an entry (v, u, w) may be cut into s entries (v, u, w_1 .. w_s) with sum llrint(w_i * 2^32) ==
llrint(w * 2^32), and a row's entries may come in any order: the graph is the same graph, the labels, cluster count and modularity must
be the same bits, and the row has moved into whichever kernel the test wants.  Everything here is plain numpy / scipy; the CPU test proves
that every form a GPU test sends is the canonical graph in fixed point, so a mismatch on the GPU is the library's."""
import numpy as np
import scipy.sparse as sp

SCALE = 4294967296.0          # LV_SCALE: weights are llrint(x * 2^32)
QUANT = 2.0 ** -16            # quantise(): weights are multiples of this, so an entry has at least 2^16 units to cut

# The row-length classes of the local moving and the reduction.  Upper edges (inclusive) of the first four classes:
#   64    one entry per lane of k_lv_move_small: with several starts two copies share a round ("pair"; `hi - lo <= 64` there)
#   128   LV_SMALL_DEG: k_lv_move_small / k_lv_emit_small, two entries per lane
#   512   LV_MID_SLOTS / 2: k_lv_move_mid in one pass (k_lv_emit_big<LV_EMIT_SLOTS> from 129 on)
#   4096  LV_MID_DEG: k_lv_move_mid in ceil(len / 512) passes; beyond it k_lv_move_big / k_lv_emit_big<LV_BIG_SLOTS>
CLASS_EDGES = (64, 128, 512, 4096)
CLASS_NAMES = ("le64", "le128", "mid1", "midP", "big")
MID_PASS_LEN = 512            # LV_MID_SLOTS / 2: entries per pass of k_lv_move_mid
EMIT_PASS_LEN = 1024          # LV_EMIT_SLOTS / 2: entries per pass of k_lv_emit_big<LV_EMIT_SLOTS>
BIG_PASS_LEN = 4096           # LV_BIG_SLOTS / 2: entries per pass of k_lv_move_big and k_lv_emit_big<LV_BIG_SLOTS>


def row_lengths(indptr):
    return np.diff(np.asarray(indptr, dtype=np.int64))


def class_counts(indptr):
    """Rows per class of the table above, by name."""
    cls = np.searchsorted(np.asarray(CLASS_EDGES), row_lengths(indptr), side="left")
    return dict(zip(CLASS_NAMES, np.bincount(cls, minlength=5).tolist()))


def pass_counts(indptr):
    """The sets of pass counts the rows of the multi-pass classes take: (k_lv_move_mid, k_lv_emit_big<2048>, k_lv_move_big / k_lv_emit_big<8192>)."""
    n = row_lengths(indptr)
    mid, big = n[(n > CLASS_EDGES[1]) & (n <= CLASS_EDGES[3])], n[n > CLASS_EDGES[3]]
    up = lambda a, d: sorted(set((-(-a // d)).tolist()))
    return up(mid, MID_PASS_LEN), up(mid, EMIT_PASS_LEN), up(big, BIG_PASS_LEN)


def quantise(A):
    """Symmetric CSC in; the same structure without the diagonal out, every weight rounded to a multiple of 2^-16 and at least 2^-16."""
    C = sp.coo_matrix(A)
    keep = C.row != C.col
    data = np.maximum(np.rint(C.data[keep].astype(np.float64) / QUANT), 1.0) * QUANT
    Q = sp.csc_matrix((data, (C.row[keep], C.col[keep])), shape=C.shape)
    Q.sum_duplicates()
    Q.sort_indices()
    assert Q.nnz == int(keep.sum()), "duplicate entries in the input"
    T = Q.T.tocsc()
    T.sort_indices()
    assert np.array_equal(Q.indptr, T.indptr) and np.array_equal(Q.indices, T.indices) and np.array_equal(Q.data, T.data), "not symmetric"
    return Q


def canonical(A):
    """(indptr int64, indices int32, x float64) of a CSC matrix as it stands."""
    return A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.astype(np.float64)


def cut_rows(A, parts, rng, shuffle=True):
    """Stored element e of CSC matrix A becomes parts[e] >= 1 positive entries whose fixed-point values add up to element e's exactly.
    The parts are uneven (random shares), so a kernel that drops or double-counts one of them changes a sum.  With `shuffle` the entries
    of every row come in random order.  Returns (indptr int64, indices int32, x float64)."""
    parts = np.asarray(parts, dtype=np.int64)
    nnz, N = A.nnz, A.shape[1]
    assert parts.shape == (nnz,) and (parts >= 1).all()
    f = np.rint(A.data.astype(np.float64) * SCALE).astype(np.int64)
    assert (f >= parts).all(), "an element has fewer fixed-point units than parts"
    first = np.concatenate([[0], np.cumsum(parts)[:-1]])
    total = int(parts.sum())
    owner = np.repeat(np.arange(nnz, dtype=np.int64), parts)
    u = rng.random(total) + 0.25                                  # shares between 1 : 5 and 5 : 1
    su = np.add.reduceat(u, first)
    spare = (f - parts)[owner]                                    # every part gets one unit, the spare ones go by share (rounded down) ...
    val = 1 + np.floor(spare * (u / su[owner])).astype(np.int64)
    val[first] += f - np.add.reduceat(val, first)                 # ... and what the rounding left over to the element's first part
    assert (val > 0).all() and np.array_equal(np.add.reduceat(val, first), f)
    row = np.repeat(np.repeat(np.arange(N, dtype=np.int64), np.diff(A.indptr)), parts)
    idx = A.indices.astype(np.int32)[owner]
    if shuffle:
        order = np.argsort(row + rng.random(total), kind="stable")
        assert np.array_equal(row[order], row)
        idx, val = idx[order], val[order]
    indptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=N))]).astype(np.int64)
    return indptr, idx, val.astype(np.float64) / SCALE            # exact: integers below 2^53 over a power of two


def parts_uniform(A, factor):
    return np.full(A.nnz, int(factor), dtype=np.int64)


def parts_per_row(A, factor_of_row):
    """Every element of row v cut into factor_of_row[v] parts."""
    return np.repeat(np.asarray(factor_of_row, dtype=np.int64), np.diff(A.indptr))


def parts_for_lengths(A, target_len, rng):
    """Parts that give row v exactly target_len[v] entries (target_len[v] < 0 or == its length: untouched): the target_len[v] - deg[v]
    extra parts are spread over the row's elements, as evenly as they go, the odd ones at random."""
    deg = np.diff(A.indptr)
    parts = np.ones(A.nnz, dtype=np.int64)
    for v in np.flatnonzero(np.asarray(target_len) >= 0):
        extra = int(target_len[v]) - int(deg[v])
        assert deg[v] > 0 and extra >= 0, "a row cannot shrink, an empty row cannot grow"
        lo, hi = A.indptr[v], A.indptr[v + 1]
        parts[lo:hi] += extra // deg[v]
        parts[lo + rng.choice(deg[v], extra % deg[v], replace=False)] += 1
    return parts


def fixed_point_matrix(indptr, indices, x, N):
    """The matrix the device sums: rint(x * 2^32) as int64, duplicates summed, indices sorted.  Two forms are the same graph iff
    these are equal (same_graph)."""
    f = np.rint(np.asarray(x, dtype=np.float64) * SCALE).astype(np.int64)
    # copies: scipy sorts the arrays it was given in place, and the caller's are the unsorted form under test
    M = sp.csc_matrix((f, np.array(indices, dtype=np.int32), np.array(indptr, dtype=np.int64)), shape=(N, N))
    M.sum_duplicates()
    M.sort_indices()
    return M


def same_graph(a, b):
    return a.shape == b.shape and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and np.array_equal(a.data, b.data)


# ---- graphs that need no device (the kNN -> Jaccard graphs of the GPU tests come from tests.test_louvain_gpu.knn_graph)
def symmetric_from_edges(N, rows, cols, vals):
    W = sp.coo_matrix((vals, (rows, cols)), shape=(N, N)).tocsc()
    A = (W + W.T).tocsc()
    A.sum_duplicates()
    A.sort_indices()
    return A


def many_hubs_graph(n_hubs=200, n_leaves=60000, lo=130, hi=9000, seed=33):
    """n_hubs hubs (vertices 0 .. n_hubs - 1) with degrees log-uniform in lo .. hi over n_leaves leaves that also sit on a ring; weights
    integers(1, 32) / 64.  At the start every neighbour of a hub is its own community: the multi-pass tables hold hundreds of distinct keys."""
    rng = np.random.default_rng(seed)
    N = n_hubs + n_leaves
    deg = np.exp(rng.uniform(np.log(lo), np.log(hi), n_hubs)).astype(np.int64)
    deg[:4] = (lo, hi, 513, 4097)                                 # both ends and both seams are there whatever the draw
    rows, cols, vals = [], [], []
    for h in range(n_hubs):
        leaves = n_hubs + rng.choice(n_leaves, int(deg[h]), replace=False)
        rows += [np.full(int(deg[h]), h)]; cols += [leaves]; vals += [rng.integers(1, 32, int(deg[h])) / 64.0]
    ring = np.arange(n_hubs, N)
    rows += [ring]; cols += [np.roll(ring, -1)]; vals += [rng.integers(1, 32, n_leaves) / 64.0]
    return symmetric_from_edges(N, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)), deg


def random_tree_edges(n, n_chords, rng):
    """A random recursive tree on n vertices (vertex i > 0 hangs on a random earlier one) plus n_chords random chords."""
    a = np.arange(1, n)
    b = (rng.random(n - 1) * a).astype(np.int64)
    if n_chords and n > 2:
        ca, cb = rng.integers(0, n, n_chords), rng.integers(0, n, n_chords)
        ok = ca != cb
        a, b = np.concatenate([a, ca[ok]]), np.concatenate([b, cb[ok]])
    return a, b


def components_graph(seed=5, n_small=300, n_isolated=50, big=(3000, 3000)):
    """n_small components of 2 .. 40 vertices, two big ones (random trees plus a few chords each), n_isolated vertices without an edge,
    the vertex ids permuted.  Returns (A, component id of every vertex, -1 for the isolated ones)."""
    rng = np.random.default_rng(seed)
    sizes = np.concatenate([rng.integers(2, 41, n_small), np.asarray(big, dtype=np.int64)])
    N = int(sizes.sum()) + n_isolated
    rows, cols, comp = [], [], np.full(N, -1, dtype=np.int64)
    at = 0
    for c, n in enumerate(sizes.tolist()):
        a, b = random_tree_edges(n, max(1, n // 4), rng)
        rows += [at + a]; cols += [at + b]
        comp[at:at + n] = c
        at += n
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    perm = rng.permutation(N)
    A = symmetric_from_edges(N, perm[rows], perm[cols], rng.integers(1, 32, len(rows)) / 64.0)
    out = np.empty(N, dtype=np.int64)
    out[perm] = comp
    return A, out


def standin_knn_graph(N, k, seed):
    """A kNN-like symmetric graph without a device (the CPU test's stand-in for the kNN -> Jaccard graphs): every vertex names k others,
    the union of both directions is kept; rows of k to about 3 k entries, weights in (0, 1]."""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(N), k)
    cols = (rows + 1 + rng.integers(0, N - 1, N * k)) % N
    lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
    pair = np.unique(lo * N + hi)
    return symmetric_from_edges(N, pair // N, pair % N, 1.0 - rng.random(len(pair)))


# ---- the forms the GPU tests send, each (indptr, indices, x) of the graph of quantised matrix A
SEAM_LENGTHS = (64, 65, 128, 129, 512, 513, 1024, 1025, 4096, 4097, 8192, 8193)
PROMOTE_LENGTHS = {"le64": 60, "le128": 100, "mid1": 300, "midP": 2000, "big": 6000}      # one row length inside every class


def form_shuffle(A, rng):
    """The same entries, every row in random order."""
    return cut_rows(A, parts_uniform(A, 1), rng)


def form_uniform(A, factor, rng):
    return cut_rows(A, parts_uniform(A, factor), rng)


def form_all_big(A, factor, rng):
    """Every row beyond CLASS_EDGES[-1] entries: every element cut into `factor` parts, and into as many as it takes where that is too few."""
    deg = np.maximum(np.diff(A.indptr), 1)
    return cut_rows(A, parts_per_row(A, np.maximum(factor, -(-(CLASS_EDGES[-1] + 1) // deg))), rng)


def form_mixed(A, rng, top=200):
    """A random factor 1 .. top per vertex: all classes side by side, neighbours in different ones."""
    return cut_rows(A, parts_per_row(A, rng.integers(1, top + 1, A.shape[0])), rng)


def form_rows(A, rows, factor, rng):
    """Only the given rows cut (every element of them into `factor` parts); all rows shuffled."""
    f = np.ones(A.shape[0], dtype=np.int64)
    f[np.asarray(rows)] = factor
    return cut_rows(A, parts_per_row(A, f), rng)


def form_seams(A, rng, per=40):
    """`per` vertices at each row length of SEAM_LENGTHS, the rest untouched.  Returns (form, target_len; -1 = untouched)."""
    deg = np.diff(A.indptr)
    ok = np.flatnonzero((deg > 0) & (deg <= SEAM_LENGTHS[0]))
    chosen = rng.choice(ok, per * len(SEAM_LENGTHS), replace=False)
    target = np.full(A.shape[0], -1, dtype=np.int64)
    target[chosen] = np.repeat(np.asarray(SEAM_LENGTHS), per)
    return cut_rows(A, parts_for_lengths(A, target, rng), rng), target


def form_promote(A, cls, rng):
    """One vertex in 50 given the row length PROMOTE_LENGTHS[cls].  Returns (form, target_len)."""
    deg = np.diff(A.indptr)
    ok = np.flatnonzero((deg > 0) & (deg <= PROMOTE_LENGTHS[cls]))
    target = np.full(A.shape[0], -1, dtype=np.int64)
    target[rng.choice(ok, A.shape[0] // 50, replace=False)] = PROMOTE_LENGTHS[cls]
    return cut_rows(A, parts_for_lengths(A, target, rng), rng), target


def nested_pairing_graph(levels):
    """2^levels vertices; for every l < levels, the first vertices of the two halves of every aligned block of 2^(l + 1) vertices are joined
    with weight 2^(10 - l): at resolution 0 every level of the descent merges exactly the sibling blocks, so the descent has `levels` levels
    that merge something (algorithm 2 keeps the vertex maps of LV_MAX_SAVED = 12 of them)."""
    N = 1 << levels
    rows, cols, vals = [], [], []
    for l in range(levels):
        left = np.arange(0, N, 2 << l)
        rows += [left]; cols += [left + (1 << l)]; vals += [np.full(len(left), 2.0 ** (10 - l))]
    return symmetric_from_edges(N, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals))
