"""Graphs of the Leiden tests (tests/test_leiden_cpu.py, tests/test_leiden_gpu.py): built without a device."""
import os

import numpy as np
import scipy.sparse as sp

from tests.helpers import closed_form

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "louvain_cases.npz")
RINGS = [(8, 5), (60, 10)]          # cliques, vertices each: 40 and 600 vertices
_golden = None


def golden():
    """name -> (A, resolution, the reference optimiser's labels) of tests/golden/louvain_cases.npz."""
    global _golden
    if _golden is None:
        z = np.load(GOLDEN)
        _golden = {}
        for n in sorted({k.split("/")[0] for k in z.files}):
            N = len(z[n + "/indptr"]) - 1
            A = sp.csc_matrix((z[n + "/data"], z[n + "/indices"], z[n + "/indptr"]), shape=(N, N))
            _golden[n] = (A, float(z[n + "/params"][0]), z[n + "/labels"])
    return _golden


def ring(c, m):
    return closed_form.ring_of_cliques(c, m)


def disconnected_start(c, m):
    """A ring of c cliques of m with cliques 0 and c / 2 given one label: a community of two components."""
    A, clique = ring(c, m)
    init = clique.astype(np.int32).copy()
    init[clique == c // 2] = 0
    return A, clique, init


def hub_graph(N=6000, hubs=((0, 5000), (1, 300))):
    """tests/test_louvain_gpu.py's hub_graph scaled down (the same generator and default_rng(21)): every leaf also on a ring."""
    rng = np.random.default_rng(21)
    rows, cols, vals = [], [], []
    for hub, deg in hubs:
        leaves = rng.choice(np.arange(2, N), deg, replace=False)
        rows += [np.full(deg, hub)]; cols += [leaves]; vals += [rng.integers(1, 32, deg) / 64.0]
    ring_ = np.arange(2, N)
    rows += [ring_]; cols += [np.roll(ring_, -1)]; vals += [np.full(N - 2, 0.5)]
    W = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N)).tocsc()
    A = (W + W.T).tocsc()
    A.sum_duplicates(); A.sort_indices()
    return A


# ---- the inputs of the exact comparison (tests/test_leiden_exact_gpu.py), qualified without a device by tests/test_leiden_par_cpu.py:
# the exact restatement (tests/helpers/leiden_par.py) counts no fragile decision on any of them
EXACT_SEEDS = (0, 1234)
STANDIN_SEEDS = (7, 8, 9)               # louvain_forms.standin_knn_graph(2100, 10, s), quantised, at resolution 0.8
ZERO_SEEDS = (8, 10, 12)                # louvain_forms.standin_knn_graph(500, 4, s), quantised, at resolution 1.0
PATH_GRAPH = "standin7"                 # the graph that tests/test_leiden_exact_gpu.py cuts into rows of chosen lengths
SEAM_LENGTHS = (128, 129, 1024, 1025, 2049)      # LD_SMALL_DEG and one beyond; one, two and three passes of LD_PASS_KEYS = 1024 keys
SEAM_ROWS = 30
_exact, _runs = None, {}


def exact_inputs():
    """name -> (A, resolution)."""
    global _exact
    if _exact is None:
        from tests.helpers import louvain_forms as lf

        _exact = {n: (A, res) for n, (A, res, _) in golden().items()}
        for c, m in RINGS:
            _exact[f"ring{c}x{m}"] = (ring(c, m)[0], 0.8)
        for s in STANDIN_SEEDS:
            _exact[f"standin{s}"] = (lf.quantise(lf.standin_knn_graph(2100, 10, s)), 0.8)
        for s in ZERO_SEEDS:
            _exact[f"small{s}"] = (lf.quantise(lf.standin_knn_graph(500, 4, s)), 1.0)
    return _exact


EXACT_NAMES = (["knn_blobs", "knn_noise_alg2", "planted3", "planted8_res08"] + [f"ring{c}x{m}" for c, m in RINGS]
               + [f"standin{s}" for s in STANDIN_SEEDS] + [f"small{s}" for s in ZERO_SEEDS])


def exact_seeds(name):
    """The seeds at which `name` is qualified (the 500-vertex graphs of the stored-zero tests: seed 0 alone, small12 is fragile at 1234)."""
    return (0,) if name.startswith("small") else EXACT_SEEDS


def exact_run(name, seed):
    """The restated run of two iterations (leiden_par.leiden: .after holds the result of one), made once per process."""
    from tests.helpers import leiden_par

    if (name, seed) not in _runs:
        A, res = exact_inputs()[name]
        _runs[name, seed] = leiden_par.leiden(A, res, 2, seed)
    return _runs[name, seed]


def with_stored_zeros(A, per_row=8, seed=0):
    """A with `per_row` stored zeros in every row, to vertices that are neither the row's neighbours nor the row itself."""
    rng = np.random.default_rng(seed)
    N = A.shape[0]
    ptr, idx, x = [0], [], []
    for v in range(N):
        own = A.indices[A.indptr[v]:A.indptr[v + 1]]
        free = np.setdiff1d(np.arange(N), np.append(own, v))
        extra = rng.choice(free, per_row, replace=False)
        idx += [own, extra]; x += [A.data[A.indptr[v]:A.indptr[v + 1]], np.zeros(per_row)]
        ptr.append(ptr[-1] + len(own) + per_row)
    B = sp.csc_matrix((np.concatenate(x), np.concatenate(idx).astype(np.int32), np.asarray(ptr, dtype=np.int64)), shape=(N, N))
    B.sort_indices()
    assert B.nnz == A.nnz + per_row * N and (B != A).nnz == 0
    return B


def with_diagonal(A, value=0.5):
    B = (A + sp.identity(A.shape[0], format="csc") * value).tocsc()
    B.sort_indices()
    assert B.nnz == A.nnz + A.shape[0]
    return B


def seam_form(A, rng):
    """SEAM_ROWS rows at each of SEAM_LENGTHS, the others as they are, all rows shuffled: (form, target length or -1)."""
    from tests.helpers import louvain_forms as lf

    deg = np.diff(A.indptr)
    chosen = rng.choice(np.flatnonzero((deg > 0) & (deg <= SEAM_LENGTHS[0])), SEAM_ROWS * len(SEAM_LENGTHS), replace=False)
    target = np.full(A.shape[0], -1, dtype=np.int64)
    target[chosen] = np.repeat(np.asarray(SEAM_LENGTHS), SEAM_ROWS)
    return lf.cut_rows(A, lf.parts_for_lengths(A, target, rng), rng), target


def all_long_form(A, rng):
    """Every row beyond 128 entries: every element of a row cut into as many parts as that takes."""
    from tests.helpers import louvain_forms as lf

    deg = np.maximum(np.diff(A.indptr), 1)
    return lf.cut_rows(A, lf.parts_per_row(A, -(-(SEAM_LENGTHS[0] + 1) // deg)), rng)


def ld_path_counts(indptr, n):
    """Rows per kernel of gficf_amd/csrc/leiden.hip at level 0, from the indptr that is sent: the wave kernel (up to 128 entries), and
    the workgroup kernel by its number of passes ceil(min(entries, n) / 1024)."""
    length = np.diff(np.asarray(indptr, dtype=np.int64))
    long_ = length[length > 128]
    passes = -(-np.minimum(long_, n) // 1024)
    return {"wave": int((length <= 128).sum()), **{int(p): int((passes == p).sum()) for p in np.unique(passes)}}
