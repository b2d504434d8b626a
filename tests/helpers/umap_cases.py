"""Inputs, property checks and layout cases shared by tests/test_umap_cpu.py (the numpy port) and tests/test_umap_gpu.py (the
library), so that both are held to the same statements.

``python -m tests.helpers.umap_cases`` recomputes, on the CPU and with the port alone, the MEASURED tables that
tests/test_umap_gpu.py and tests/test_umap_exact_gpu.py carry (the f32 / f64 deviation of every layout case, the port's quality
figures)."""
import functools

import numpy as np
import scipy.sparse as sp

from tests.helpers import umap_np as un

GRAPH_KS = (2, 5, 15, 64, 128)


# ------------------------------------------------------------------------------------------------ inputs
def graph_input():
    """300 points in 10-D: 99 random ones, a block of 20 identical points (rho = 0 and the global-mean floor for k <= 20), a
    centre far from the rest with the 180 points centre + (+-1, +-1, 0, ...) around it, all at the distance sqrt(2) from it in
    exact f32 arithmetic: the centre's row holds one distance only, for every k <= 128."""
    rng = np.random.default_rng(11)
    X = [rng.standard_normal((99, 10)), np.tile(rng.standard_normal((1, 10)), (20, 1))]
    centre = np.zeros(10)
    centre[0] = 50.0
    shell = []
    for p in range(10):
        for q in range(p + 1, 10):
            for sa in (1.0, -1.0):
                for sb in (1.0, -1.0):
                    v = centre.copy()
                    v[p] += sa
                    v[q] += sb
                    shell.append(v)
    X += [centre[None, :], np.array(shell)]
    X = np.concatenate(X)
    assert X.shape == (300, 10)
    return X


GRAPH_CENTRE = 119                  # the row of graph_input() whose distances are all equal
GRAPH_BLOCK = slice(99, 119)        # its identical points


def random_input(n=257, dim=10, seed=5):
    return np.random.default_rng(seed).standard_normal((n, dim))


def hub_points(n=2000, dim=10, seed=3):
    """n points on the unit sphere and the origin (the last row)."""
    U = np.random.default_rng(seed).standard_normal((n, dim))
    U /= np.linalg.norm(U, axis=1, keepdims=True)
    return np.concatenate([U, np.zeros((1, dim))])


def hub_table(idx, dist):
    """The neighbour table of hub_points() in which every point names the origin.  About 117 of 2 000 random points of the unit
    sphere in 10-D lie within 60 degrees of a given one and so closer to it than the origin is (no 2 000 points of that sphere
    are pairwise further apart than 1: the kissing number of 10-D is below 600), so an exact table never names the origin.
    This is the table an approximate search may return: the last column of every sphere point's row is replaced by the origin
    at its true distance, which keeps the row ascending.  One row of the graph then has an entry for every other point."""
    idx, dist = np.array(idx), np.array(dist, dtype=np.float32)
    N = idx.shape[0]
    origin = N                                                   # 1-based id of the last row
    assert not (idx[:-1] == origin).any()
    to_origin = np.ones(N - 1, dtype=np.float32)
    assert (dist[:-1, -1] <= to_origin).all()
    idx[:-1, -1] = origin
    dist[:-1, -1] = to_origin
    return idx, dist


def plane_init(X):
    """The first two coordinates scaled to a largest magnitude of 10 (what init='pca' does, without its noise)."""
    Y = np.array(X[:, :2], dtype=np.float64)
    return Y * (10.0 / np.abs(Y).max())


# ------------------------------------------------------------------------------------------------ the graph's defining properties
def check_graph(idx, dist, P, sigma, rho, W, mix=1.0, lc=1.0):
    """Everything in f64 from the given sigma and rho: no second implementation in the loop."""
    idx = np.asarray(idx)
    N, k = idx.shape
    d32 = np.maximum(np.asarray(dist, dtype=np.float32), np.float32(0))     # a distance rounded below 0 counts as 0
    d = d32.astype(np.float64)
    sigma32, rho32, W = np.asarray(sigma, np.float32), np.asarray(rho, np.float32), np.asarray(W, np.float32)
    assert sigma32.shape == (N,) and rho32.shape == (N,) and W.shape == (N, k)
    sig, rh = sigma32.astype(np.float64), rho32.astype(np.float64)
    # rho: the selected input distance, exactly
    f = int(np.floor(lc))
    r = np.float32(lc - f)
    for i in range(N):
        nz = d32[i, 1:][d32[i, 1:] > 0]
        if len(nz) >= f:
            want = nz[f - 1]
            if r > 0 and len(nz) > f:
                want = np.float32(nz[f - 1] + r * np.float32(nz[f] - nz[f - 1]))
                assert abs(float(rho32[i]) - float(want)) <= 2 * np.spacing(want), (i, rho32[i], want)
                continue
        elif len(nz) > 0:
            want = nz.max()
        else:
            want = np.float32(0)
        assert rho32[i] == want, (i, rho32[i], want)
    # sigma: on its floor, or the sum meets its target
    slack = (k + 8) * 2.0 ** -24
    floor = 1e-3 * np.where(rh > 0, d.mean(axis=1), d.mean())
    assert (sig >= floor * (1 - slack)).all()
    x = np.maximum(d[:, 1:] - rh[:, None], 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        S = np.where(x > 0, np.exp(-x / sig[:, None]), 1.0).sum(axis=1)
    target, bound = np.log2(k), 1e-5 + k * 2.0 ** -21
    on_floor = sig <= floor * (1 + slack)
    ok = (np.abs(S - target) <= bound) | (on_floor & (S >= target - bound))
    assert ok.all(), (np.flatnonzero(~ok)[:5], S[~ok][:5], target)
    # memberships
    xa = d - rh[:, None]
    own = idx == np.arange(1, N + 1)[:, None]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w64 = np.where(own, 0.0, np.where(xa <= 0, 1.0, np.exp(-xa / sig[:, None])))
    assert np.abs(W.astype(np.float64) - w64).max() <= 2.0 ** -21
    assert (W[own] == 0).all() and (W[~own & (xa <= 0)] == 1).all()
    # P against the memberships it was made of
    rows = np.repeat(np.arange(N), k)
    cols = idx.ravel().astype(np.int64) - 1
    wv = W.ravel().astype(np.float64)
    A = sp.csr_matrix((wv[wv > 0], (rows[wv > 0], cols[wv > 0])), shape=(N, N))
    AT = A.T.tocsr()
    had = A.multiply(AT)
    E = (mix * (A + AT - had) + (1.0 - mix) * had).tocsr()
    E.eliminate_zeros()
    E.sort_indices()
    P = sp.csr_matrix(P)
    assert P.dtype == np.float32 and P.shape == (N, N)
    assert P.indptr[0] == 0 and P.indptr[-1] == len(P.indices) == len(P.data)
    for i in range(N):
        c = P.indices[P.indptr[i]:P.indptr[i + 1]]
        assert (np.diff(c) > 0).all(), i                         # ascending, no repeats
        assert not (c == i).any(), i                             # no diagonal
    assert (P.data > 0).all()
    assert np.array_equal(P.indptr, E.indptr) and np.array_equal(P.indices, E.indices)
    if mix == 1.0:
        S2 = (A + AT).tocsr()
        S2.sort_indices()
        assert np.array_equal(P.indptr, S2.indptr) and np.array_equal(P.indices, S2.indices)
    ulp = np.spacing(E.data.astype(np.float32)).astype(np.float64)
    assert (np.abs(P.data.astype(np.float64) - E.data) <= 4 * ulp).all()
    PT = P.T.tocsr()
    PT.sort_indices()
    assert np.array_equal(PT.indptr, P.indptr) and np.array_equal(PT.indices, P.indices)
    assert np.array_equal(PT.data.view(np.uint32), P.data.view(np.uint32))        # P == P' bit for bit
    return P


# ------------------------------------------------------------------------------------------------ layout cases
AB = {"tumap": (1.0, 1.0), "umap": (1.8956, 0.8006)}
RANGES = {"0-1": (0, 1), "100-101": (100, 101), "0-3": (0, 3)}
LAYOUT_EPOCHS = 200
LAYOUT_SEED = 42
FLOOR = 64 * 2.0 ** -24 * 10                                     # 64 f32 roundings at the largest coordinate, 10


@functools.lru_cache(maxsize=None)
def layout_graph(name):
    """(P, Y0) of the layout cases, made by the port: "rand" 257 random points, "hub" the 2 001-point hub graph."""
    if name == "rand":
        X = random_input()
        idx, dist = un.exact_knn(X, 15)
    else:
        X = hub_points()
        idx, dist = hub_table(*un.exact_knn(X, 15))
    P, _, _ = un.fuzzy_graph(idx, dist)
    if name == "hub":
        assert np.diff(P.indptr).max() == P.shape[0] - 1         # the origin's row names every other point
    return P, plane_init(X)


def crafted():
    """257 random points of which 50 start at the same coordinates: the d2 == 0 branches of both forces."""
    P, Y0 = layout_graph("rand")
    Y0 = Y0.copy()
    Y0[100:150] = Y0[100]
    return P, Y0


def port_layout(name, ab, rng_name, dtype):
    P, Y0 = crafted() if name == "crafted" else layout_graph(name)
    a, b = AB[ab]
    lo, hi = RANGES[rng_name]
    return un.layout(P, Y0, LAYOUT_EPOCHS, a, b, 1.0, 1.0, 5, LAYOUT_SEED, lo, hi, dtype)


def layout_cases():
    cases = [(g, ab, r) for g in ("rand", "hub") for ab in AB for r in RANGES]
    return cases + [("crafted", "tumap", "100-101")]


def tolerance(measured):
    return max(8.0 * measured, FLOOR)


# ------------------------------------------------------------------------------------------------ exact cases: crafted shapes
# What tests/test_umap_exact_gpu.py holds to the bits of the float32 port, and tests/test_umap_cpu.py keeps from being vacuous.
HUB_LEN = 256                        # UM_HUB_LEN of umap.hip: a longer row is walked by a whole wave, 64 entries a round
GROUP, WAVE = 8, 64                  # lanes per vertex on the two paths
HUB_WAVES = 1024                     # UM_HUB_WAVES: with more hubs than this a wave takes a second one
SEAM_LENGTHS = (0, 1, 2, 7, 8, 9, 15, 16, 17, 24, 25, 63, 64, 65, 255, 256, 257, 258, 299, 0)      # rows 0 .. 19 of seams()
SEAM_SHARED = slice(100, 130)        # the vertices of seams() that start at one position; their rows name each other only
SEAM_RATES = (0, 1, 5, 7, 8, 9, 16, 17, 63, 64, 65, 130)
WINDOWS = {"0-1": (0, 1), "100-101": (100, 101), "100-102": (100, 102), "100-103": (100, 103), "0-3": (0, 3)}
PAD_VALUE = 1e-12                    # a value whose schedule word is 0 beside a largest value of 0.05 or more
PADDED = ((256, 1), (200, 57), (200, 130))
PADDED_RATES = (0, 5, 65)
PADDED_N, PADDED_WINDOW = 400, "100-102"


def shape_graph(lengths, seed, pools=None):
    """A CSR matrix whose row i has lengths[i] distinct ascending columns other than i, drawn from pools[i] where that is given
    and from all vertices otherwise, with float32 values uniform in [0.05, 1] (an entry of value w is due in about w / wmax of
    the epochs: roughly half of them in any one).  Not symmetric: the layout reads rows only."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    N = len(lengths)
    cols = []
    for i, n in enumerate(lengths):
        pool = np.setdiff1d(np.arange(N) if pools is None or i not in pools else pools[i], [i])
        cols.append(np.sort(rng.choice(pool, size=int(n), replace=False)))
    indices = np.concatenate(cols).astype(np.int32)
    data = rng.uniform(0.05, 1.0, size=len(indices)).astype(np.float32)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return sp.csr_matrix((data, indices, indptr), shape=(N, N))


@functools.lru_cache(maxsize=None)
def seams():
    """(P, Y0), 300 vertices.  Rows 0 .. 19 have the lengths SEAM_LENGTHS: empty, shorter than, as long as and longer than one
    and two rounds of a group, both sides of the hub threshold, every other vertex; the rest 0 .. 19 entries.  Y0 is uniform in
    [-10, 10] except for the 30 vertices of SEAM_SHARED, which start at one position and whose rows name each other only: their
    attractions run at d2 == 0 and leave them in place, so that a negative sample among them is a repulsion at d2 == 0."""
    rng = np.random.default_rng(101)
    N = 300
    lengths = np.concatenate([SEAM_LENGTHS, rng.integers(0, 20, size=N - len(SEAM_LENGTHS))])
    shared = np.arange(N)[SEAM_SHARED]
    P = shape_graph(lengths, 102, pools={int(v): shared for v in shared})
    # the last entry of the row of 257 is alone in the fifth round of its wave; at the smallest value it is due in epochs 19,
    # 39, .., 99, 119 only, so in the tested epochs the wave path meets a round with nothing due (64 entries never all rest)
    P.data[P.indptr[SEAM_LENGTHS.index(257) + 1] - 1] = 0.05
    Y0 = rng.uniform(-10.0, 10.0, size=(N, 2))
    Y0[SEAM_SHARED] = Y0[SEAM_SHARED.start]
    return P, Y0


@functools.lru_cache(maxsize=None)
def many_hubs():
    """(P, Y0), 1 100 vertices: 1 030 rows of 257 + (h mod 44) entries, h the hub's ordinal, and 70 rows of 0 .. 19 entries spread
    among them: more hubs than HUB_WAVES, so the stride loop over the hub list makes a second round."""
    rng = np.random.default_rng(201)
    N = 1100
    short = np.linspace(0, N - 1, 70).astype(np.int64)
    lengths = np.zeros(N, dtype=np.int64)
    is_hub = np.ones(N, dtype=bool)
    is_hub[short] = False
    lengths[is_hub] = 257 + np.arange(is_hub.sum()) % 44
    lengths[short] = rng.integers(0, 20, size=len(short))
    return shape_graph(lengths, 202), rng.uniform(-10.0, 10.0, size=(N, 2))


@functools.lru_cache(maxsize=None)
def padded(L, pad):
    """(P, Y0, v), PADDED_N vertices: rows of 0 .. 19 entries, and the last row v with L entries at columns below PADDED_N - 131
    followed by ``pad`` entries of value PAD_VALUE at the columns from there on.  The padding has schedule word 0, is never due,
    and, coming last in the last row, shifts no entry index: padded(L, pad) and padded(L, 0) differ in the length of row v only."""
    N = PADDED_N
    v, first_pad = N - 1, N - 131
    assert 0 <= pad <= v - first_pad and 0 < L <= first_pad
    rng = np.random.default_rng(301)
    lengths = np.concatenate([rng.integers(0, 20, size=N - 1), [0]])
    base = shape_graph(lengths, 302)
    Y0 = rng.uniform(-10.0, 10.0, size=(N, 2))
    row = np.random.default_rng(303 + L)
    cols = np.concatenate([np.sort(row.choice(first_pad, size=L, replace=False)), first_pad + np.arange(pad)])
    vals = np.concatenate([row.uniform(0.05, 1.0, size=L), np.full(pad, PAD_VALUE)])
    indptr = base.indptr.astype(np.int64).copy()
    indptr[-1] += L + pad
    P = sp.csr_matrix((np.concatenate([base.data, vals]).astype(np.float32), np.concatenate([base.indices, cols]).astype(np.int32), indptr),
                      shape=(N, N))
    return P, Y0, v


def exact_graph(name):
    if name == "seams":
        return seams()
    if name == "many_hubs":
        return many_hubs()
    return crafted() if name == "crafted" else layout_graph(name)


def exact_cases():
    """(graph, window, negative_sample_rate), all on the t-UMAP curve with LAYOUT_EPOCHS epochs and LAYOUT_SEED."""
    cases = [("seams", "100-101", r) for r in SEAM_RATES]
    cases += [("seams", "0-1", 5), ("seams", "100-103", 5), ("many_hubs", "100-102", 5)]
    return cases + [(g, r, 5) for g in ("rand", "hub") for r in RANGES] + [("crafted", "100-101", 5)]


def exact_id(case):
    return "-".join(str(c) for c in case)


@functools.lru_cache(maxsize=None)
def exact_port(graph, window, rate, dtype=np.float32):
    """The port's result of an exact case in ``dtype``; computed once, not to be written to."""
    P, Y0 = exact_graph(graph)
    lo, hi = WINDOWS[window]
    Y = un.layout(P, Y0, LAYOUT_EPOCHS, 1.0, 1.0, 1.0, 1.0, rate, LAYOUT_SEED, lo, hi, dtype)
    Y.setflags(write=False)
    return Y


def entry_rows(P):
    """(row, position within the row) of every entry."""
    length = np.diff(P.indptr)
    rows = np.repeat(np.arange(P.shape[0]), length)
    return rows, np.arange(len(rows)) - P.indptr[rows]


def round_coverage(P, n):
    """Per path (GROUP: rows of up to HUB_LEN entries, WAVE: longer ones), what the schedule of epoch n does to the rounds of G
    entries a row is fetched in: ``first`` / ``last``: a due entry sits in lane slot 0 / G - 1; ``ragged``: a due entry sits in
    a last round of fewer than G entries; ``empty``: some round has no due entry; ``rows``: the rows on that path."""
    fire = un.due(un.schedule(P.data), n)
    length = np.diff(P.indptr)
    rows, pos = entry_rows(P)
    out = {}
    for G, sel in ((GROUP, length[rows] <= HUB_LEN), (WAVE, length[rows] > HUB_LEN)):
        slot, rnd = pos % G, pos // G
        in_ragged = rnd == length[rows] // G                     # a last round that is not full (pos < length)
        rid = rows * (P.shape[0] + 1) + rnd
        out[G] = dict(first=bool((sel & fire & (slot == 0)).any()), last=bool((sel & fire & (slot == G - 1)).any()),
                      ragged=bool((sel & fire & in_ragged).any()), empty=len(np.unique(rid[sel & fire])) < len(np.unique(rid[sel])),
                      rows=int(((length <= HUB_LEN) if G == GROUP else (length > HUB_LEN)).sum()))
    return out


def sample_ids(P, n, rate, seed=LAYOUT_SEED):
    """(entries due in epoch n, their rows, their negative samples as a len x rate table), by the key of include/gficf_umap.h."""
    e = np.flatnonzero(un.due(un.schedule(P.data), n))
    rows, _ = entry_rows(P)
    N = np.uint64(P.shape[0])
    with np.errstate(over="ignore"):
        ke = un.mix(un.mix(np.uint64((int(seed) + n) & 0xFFFFFFFFFFFFFFFF)) + e.astype(np.uint64))
        jn = [((un.mix(ke + np.uint64(s)) >> np.uint64(32)) * N) >> np.uint64(32) for s in range(rate)]
    return e, rows[e], np.stack(jn, axis=1).astype(np.int64) if rate else np.zeros((len(e), 0), dtype=np.int64)


def self_samples(P, n, rate, seed=LAYOUT_SEED):
    """How many negative samples of epoch n name their own vertex: the ``jn != v`` skip."""
    _, rows, jn = sample_ids(P, n, rate, seed)
    return int((jn == rows[:, None]).sum())


def seams_zero_distance(n, rate, seed=LAYOUT_SEED):
    """(attractions, repulsions) at d2 == 0 that epoch n is certain to hold when it starts from seams()'s Y0: a due entry between
    two vertices of SEAM_SHARED; and, for such a vertex, a sample among the others of SEAM_SHARED before anything has moved it
    (every attraction of its row leaves it in place, a sample naming the vertex itself is skipped, any other sample ends the walk)."""
    P, _ = seams()
    e, rows, jn = sample_ids(P, n, rate, seed)
    lo, hi = SEAM_SHARED.start, SEAM_SHARED.stop
    inside = (rows >= lo) & (rows < hi)
    assert ((P.indices[e[inside]] >= lo) & (P.indices[e[inside]] < hi)).all()
    repulsions = 0
    for v in range(lo, hi):
        moved = False
        for t in np.flatnonzero(rows == v):                        # the due entries of row v in row order
            for j in jn[t]:
                if j == v:
                    continue
                repulsions += lo <= j < hi                         # the first sample that is applied: it moves v either way
                moved = True
                break
            if moved:
                break
    return int(inside.sum()), int(repulsions)


# ------------------------------------------------------------------------------------------------ quality
QUALITY_SEEDS = (1, 2, 3, 4, 5)
QUALITY_EPOCHS = 200


@functools.lru_cache(maxsize=None)
def quality_input():
    """(X, labels, cells): the 1 200 x 20 blobs, and their PCA scores (all 20), whose first two columns are the PCA plane."""
    X, labels = un.blobs()
    Xc = X - X.mean(axis=0)
    _, _, vt = np.linalg.svd(Xc, full_matrices=False)
    return X, labels, Xc @ vt.T


def _main():
    from gficf_amd.api import umap_init

    print("MEASURED = {")
    for case in layout_cases():
        dev = float(np.abs(port_layout(*case, np.float32).astype(np.float64) - port_layout(*case, np.float64)).max())
        print(f"    {case!r}: {dev:.3e},")
    print("}")
    print("MEASURED_EXACT = {      # case: (vertices compared, |port f32 - port f64|)")
    for case in exact_cases():
        f32 = exact_port(*case, np.float32)
        print(f"    {case!r}: ({len(f32)}, {float(np.abs(f32.astype(np.float64) - exact_port(*case, np.float64)).max()):.3e}),")
    print("}")
    X, labels, cells = quality_input()
    print("initial plane:", un.quality(X, cells[:, :2], labels))
    idx, dist = un.exact_knn(cells, 15)
    print("MEASURED_QUALITY = {")
    for red in AB:
        out = []
        for s in QUALITY_SEEDS:
            Y, _ = un.umap(idx, dist, umap_init("pca", cells, len(cells), s), QUALITY_EPOCHS, *AB[red], seed=s)
            out.append(un.quality(X, Y, labels))
        print(f"    {red!r}: {out!r},")
    print("}")


if __name__ == "__main__":
    _main()
