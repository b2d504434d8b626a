"""Inputs, property checks, layout cases and device drivers shared by tests/test_transform_cpu.py (the numpy port) and
tests/test_transform_gpu.py (the library), so that both are held to the same statements.

``python -m tests.helpers.transform_cases`` recomputes, on the CPU and with the port alone, the MEASURED tables that
tests/test_transform_gpu.py and tests/test_transform_exact_gpu.py carry (the f32 / f64 deviation of every layout case, the
port's hold-out figures)."""
import functools

import numpy as np

from tests.helpers import transform_np as tn
from tests.helpers import umap_cases as uc
from tests.helpers import umap_np as un

MEMBERSHIP_KS = (2, 15, 128)
MEMBERSHIP_LCS = (1.0, 1.5, 2.0)
ROW_EQUAL, ROW_ZERO = 5, 9           # rows of membership_table() with k equal distances / k zero distances


# ------------------------------------------------------------------------------------------------ memberships
def membership_table(k):
    """(idx, dist, N): 300 queries against 400 random training points in 10-D (euclidean, by the port's brute force), with row
    ROW_EQUAL set to k equal distances and row ROW_ZERO to k zeros."""
    X = uc.random_input(400, seed=21)
    Q = uc.random_input(300, seed=22)
    idx, dist = tn.query_knn(X, Q, k)
    dist = dist.copy()
    dist[ROW_EQUAL] = dist[ROW_EQUAL, 0]
    dist[ROW_ZERO] = 0.0
    return idx, dist, len(X)


def check_memberships(dist, sigma, rho, W, lc=1.0):
    """Everything in f64 from the given sigma and rho: no second implementation in the loop.  The tolerances are those of
    umap_cases.check_graph for the same quantities."""
    d32 = np.maximum(np.asarray(dist, dtype=np.float32), np.float32(0))
    d = d32.astype(np.float64)
    M, k = d.shape
    sigma32, rho32, W = np.asarray(sigma, np.float32), np.asarray(rho, np.float32), np.asarray(W, np.float32)
    assert sigma32.shape == (M,) and rho32.shape == (M,) and W.shape == (M, k)
    sig, rh = sigma32.astype(np.float64), rho32.astype(np.float64)
    cp = max(0.0, lc - 1.0)
    f = int(np.floor(cp))
    r = np.float32(cp - f)
    for i in range(M):
        nz = d32[i][d32[i] > 0]
        if f == 0:
            want = np.float32(r * nz[0]) if len(nz) else np.float32(0)
            assert abs(float(rho32[i]) - float(want)) <= (2 * np.spacing(want) if r > 0 else 0), (i, rho32[i], want)
            continue
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
    # sigma: on its floor (the row's own mean), or the sum over ALL k columns meets its target
    slack = (k + 8) * 2.0 ** -24
    floor = 1e-3 * d.mean(axis=1)
    assert (sig >= floor * (1 - slack)).all()
    x = np.maximum(d - rh[:, None], 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        S = np.where(x > 0, np.exp(-x / sig[:, None]), 1.0).sum(axis=1)
    target, bound = np.log2(k), 1e-5 + k * 2.0 ** -21
    on_floor = sig <= floor * (1 + slack)
    flat = (x > 0).sum(axis=1) == 0                              # no column beyond rho: the sum is k whatever sigma is
    ok = (np.abs(S - target) <= bound) | (on_floor & (S >= target - bound)) | (flat & (S == k))
    assert ok.all(), (np.flatnonzero(~ok)[:5], S[~ok][:5], target)
    xa = d - rh[:, None]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w64 = np.where(xa <= 0, 1.0, np.exp(-xa / sig[:, None]))
    assert np.abs(W.astype(np.float64) - w64).max() <= 2.0 ** -21
    assert (W[xa <= 0] == 1).all()
    return S


# ------------------------------------------------------------------------------------------------ layout cases
AB = uc.AB
RANGES = {"0-1": (0, 1), "30-31": (30, 31), "0-3": (0, 3)}
LAYOUT_EPOCHS = 67
LAYOUT_SEED = 42
LAYOUT_K = 15
LAYOUT_LR = 0.25                    # the transform's default learning rate
CRAFTED = slice(100, 150)           # the new cells of the crafted case that start on their nearest trained cell
CRAFTED_EPOCH = "30-31"
FLOOR = uc.FLOOR                                                 # 64 f32 roundings at the largest coordinate, 10
RATES = (0, 1, 8, 9, 20)


@functools.lru_cache(maxsize=None)
def layout_case(name, k=LAYOUT_K):
    """(idx, W, Y_train, Y0) by the port: 500 new cells against a trained layout of 1 500 points (umap_cases.random_input and
    plane_init at that size: the recipe of umap_cases.layout_graph("rand")), k neighbours each.  "crafted": the cells of CRAFTED
    start exactly on the trained cell of their column 0, whose entry has the row's largest membership and so is due in every
    epoch but the first."""
    X = uc.random_input(1500)
    Yt = uc.plane_init(X).astype(np.float32)
    Q = uc.random_input(500, seed=6)
    idx, dist = tn.query_knn(X, Q, k)
    _, _, W = tn.memberships(dist)
    Y0 = tn.init_positions(idx, W, Yt)
    if k == 1:                       # the weighted mean of one head is that head, and a cell on its only head moves by samples alone:
        Y0 = layout_case("rand")[3]  # a given start instead (umap_transform takes one), that of the case with LAYOUT_K neighbours
    if name == "crafted":
        Y0 = Y0.copy()
        Y0[CRAFTED] = Yt[idx[CRAFTED, 0] - 1]
    return idx, W, Yt, Y0


def layout_cases():
    return [("rand", ab, r) for ab in AB for r in RANGES] + [("crafted", "tumap", CRAFTED_EPOCH)]


def port_layout(name, ab, rng_name, dtype, **kw):
    idx, W, Yt, Y0 = layout_case(name)
    a, b = AB[ab]
    lo, hi = RANGES[rng_name]
    return tn.layout(idx, W, Yt, Y0, LAYOUT_EPOCHS, a, b, 1.0, LAYOUT_LR, 5, LAYOUT_SEED, 0, lo, hi, dtype, **kw)


def rate_kw(rate):
    return dict(learning_rate=LAYOUT_LR, negative_sample_rate=rate, seed=3, epoch_begin=30, epoch_end=32)


def tolerance(measured):
    return max(8.0 * measured, FLOOR)


# ------------------------------------------------------------------------------------------------ exact cases
# What tests/test_transform_exact_gpu.py holds to the bits of the float32 port, and tests/test_transform_cpu.py keeps from being
# vacuous: layout_case() at the k around the 8 lanes of a group, cut to M cells around the 8 cells of a workgroup.
GROUP = 8                            # TR_GROUP of transform.hip: lanes per new cell, and cells per workgroup
EXACT_KS = (1, 7, 8, 9, 16, 17, 128)
EXACT_MS = (1, 7, 8, 9, 500)
EXACT_RATES = (0, 7, 8, 9, 17)
EXACT_WINDOW = (30, 32)              # two epochs: the running position is carried from one to the next in registers
EXACT_SEED = 3
EXACT_CRAFTED_K = 8
EXACT_OFFSETS = ((250, 250), (0, 2 ** 40 + 3))      # (first row of the block, its query_offset)
INIT_KS = (1, 2, 15, 128)
INIT_ZERO_ROW = 3


def exact_kw(rate, query_offset=0):
    lo, hi = EXACT_WINDOW
    return dict(learning_rate=LAYOUT_LR, negative_sample_rate=rate, seed=EXACT_SEED, query_offset=query_offset, epoch_begin=lo, epoch_end=hi)


@functools.lru_cache(maxsize=None)
def exact_port(name, k, rate, dtype=np.float32, first=0, query_offset=0):
    """The port's result, in ``dtype``, for the rows from ``first`` on of layout_case(name, k) on the t-UMAP curve; computed
    once, not to be written to.  Cell i of it depends on row i and query_offset + i only (include/gficf_transform.h; the port's
    own statement of that is tests/test_transform_cpu.py), so its first M rows are the result for the first M rows."""
    idx, W, Yt, Y0 = layout_case(name, k)
    Y = tn.layout(idx[first:], W[first:], Yt, Y0[first:], LAYOUT_EPOCHS, dtype=dtype, **exact_kw(rate, query_offset))
    Y.setflags(write=False)
    return Y


def exact_cases():
    """(input, k, negative_sample_rate): every k at every rate, and the crafted coincidence at k = 8."""
    return [("rand", k, r) for k in EXACT_KS for r in EXACT_RATES] + [("crafted", EXACT_CRAFTED_K, r) for r in (0, 7)]


def round_coverage(W, n):
    """What the row-local schedule of epoch n does to the rounds of GROUP columns a row is walked in: ``first`` / ``last``: a due
    entry sits in lane slot 0 / GROUP - 1; ``ragged``: a due entry sits in a last round of fewer than GROUP columns; ``empty``:
    some round of some row has no due entry."""
    M, k = W.shape
    fire = np.stack([tn.due(tn.row_schedule(W)[:, c], n) for c in range(k)], axis=1)
    c = np.arange(k)
    per_round = np.add.reduceat(fire.astype(np.int64), np.arange(0, k, GROUP), axis=1)
    return dict(first=bool(fire[:, c % GROUP == 0].any()), last=bool(fire[:, c % GROUP == GROUP - 1].any()),
                ragged=bool(fire[:, c // GROUP == k // GROUP].any()), empty=bool((per_round == 0).any()))


@functools.lru_cache(maxsize=None)
def init_case(k):
    """(idx, W, Y_train): 300 new cells (two workgroups of the one-lane-per-cell kernel) against 400 trained ones; memberships
    uniform in (0, 1] with a tenth of them 0, and row INIT_ZERO_ROW all 0: the plain mean."""
    rng = np.random.default_rng(500 + k)
    N, M = 400, 300
    idx = np.stack([rng.choice(N, size=k, replace=False) for _ in range(M)]).astype(np.int32) + 1
    W = (1.0 - rng.random((M, k))).astype(np.float32)
    W[rng.random((M, k)) < 0.1] = 0.0
    W[INIT_ZERO_ROW] = 0.0
    return idx, W, rng.uniform(-10.0, 10.0, size=(N, 2)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ hold-out
QUALITY_SEEDS = (1, 2, 3, 4, 5)
QUALITY_EPOCHS = 200


@functools.lru_cache(maxsize=None)
def holdout():
    """(cells_train 1000 x 20, labels_train, cells_new 200 x 20, labels_new, X_train, X_new): umap_np.blobs() cut by a fixed
    permutation; the PCA scores are those of the trained cells (as umap_cases.quality_input makes them), the new cells projected."""
    X, labels = un.blobs()
    perm = np.random.default_rng(7).permutation(len(X))
    tr, te = perm[:1000], perm[1000:]
    mean = X[tr].mean(axis=0)
    _, _, vt = np.linalg.svd(X[tr] - mean, full_matrices=False)
    return (X[tr] - mean) @ vt.T, labels[tr], (X[te] - mean) @ vt.T, labels[te], X[tr], X[te]


def share(Y_train, labels_train, Y_new, labels_new, k=15):
    """The share of each new cell's k nearest TRAINED cells in the plane that carry its label."""
    A, B = np.asarray(Y_new, dtype=np.float64), np.asarray(Y_train, dtype=np.float64)
    D = ((A[:, None, :] - B[None, :, :]) ** 2).sum(-1)
    nn = np.argsort(D, axis=1, kind="stable")[:, :k]
    return float((labels_train[nn] == labels_new[:, None]).mean())


# ------------------------------------------------------------------------------------------------ device drivers (GPU tests)
@functools.lru_cache(maxsize=None)
def _ops():
    from gficf_amd.api import HipOps

    return HipOps(0)


def _cm(a, dtype):
    """An M x k host table as the (k, M) device tensor that is its column-major form."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).T, dtype=dtype)).to("cuda:0")


def _ws(stage, M, N=0, k=1):
    import torch

    return torch.empty(max(_ops().transform_workspace_bytes(stage, M, N, k), 1), dtype=torch.uint8, device="cuda:0")


def dev_weights(idx, dist, N, lc=1.0):
    import torch

    ops, (M, k) = _ops(), np.shape(idx)
    w = torch.empty((k, M), dtype=torch.float32, device="cuda:0")
    sigma, rho = (torch.empty(M, dtype=torch.float32, device="cuda:0") for _ in range(2))
    ws = _ws("weights", M, k=k)
    ops.transform_weights(_cm(idx, np.int32), _cm(dist, np.float32), N, M, k, ws, w, lc, sigma, rho)
    ops.transform_sync(ws)
    return np.ascontiguousarray(w.cpu().numpy().T), sigma.cpu().numpy(), rho.cpu().numpy()


def dev_init(idx, W, Y_train):
    import torch

    ops, (M, k) = _ops(), np.shape(idx)
    Yt = torch.from_numpy(np.ascontiguousarray(Y_train, dtype=np.float32)).to("cuda:0")
    Y = torch.empty((M, 2), dtype=torch.float32, device="cuda:0")
    ws = _ws("init", M, k=k)
    ops.transform_init(_cm(idx, np.int32), _cm(W, np.float32), Yt, len(Y_train), M, k, ws, Y)
    ops.transform_sync(ws)
    return Y.cpu().numpy()


def dev_layout(idx, W, Y_train, Y0, n_epochs, a=1.0, b=1.0, gamma=1.0, learning_rate=1.0, negative_sample_rate=5, seed=0, query_offset=0,
               epoch_begin=0, epoch_end=None):
    import torch

    ops, (M, k) = _ops(), np.shape(idx)
    Yt = torch.from_numpy(np.ascontiguousarray(Y_train, dtype=np.float32)).to("cuda:0")
    Y = torch.from_numpy(np.ascontiguousarray(Y0, dtype=np.float32)).to("cuda:0")
    ws = _ws("layout", M, k=k)
    ops.transform_layout(_cm(idx, np.int32), _cm(W, np.float32), Yt, len(Y_train), M, k, a, b, gamma, learning_rate, negative_sample_rate, n_epochs,
                         epoch_begin, n_epochs if epoch_end is None else epoch_end, seed, query_offset, Y, ws)
    ops.transform_sync(ws)
    return Y.cpu().numpy()


def dev_vote(idx, labels, C, want_votes=False):
    import torch

    ops, (M, k) = _ops(), np.shape(idx)
    lab = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to("cuda:0")
    pred = torch.empty(M, dtype=torch.int32, device="cuda:0")
    votes = torch.empty((M, C), dtype=torch.int32, device="cuda:0") if want_votes else None
    ws = _ws("vote", M, k=k)
    ops.transform_vote(_cm(idx, np.int32), lab, len(labels), M, k, C, ws, pred, votes)
    ops.transform_sync(ws)
    return (pred.cpu().numpy(), votes.cpu().numpy()) if want_votes else pred.cpu().numpy()


def dev_layout_case(name, ab, rng_name, **kw):
    idx, W, Yt, Y0 = layout_case(name)
    a, b = AB[ab]
    lo, hi = RANGES[rng_name]
    return dev_layout(idx, W, Yt, Y0, LAYOUT_EPOCHS, a, b, 1.0, LAYOUT_LR, 5, LAYOUT_SEED, 0, lo, hi, **kw), Y0


# ------------------------------------------------------------------------------------------------ the measured tables
def _main():
    from gficf_amd.api import umap_init

    print("MEASURED = {")
    for case in layout_cases():
        dev = float(np.abs(port_layout(*case, np.float32).astype(np.float64) - port_layout(*case, np.float64)).max())
        print(f"    {case!r}: {dev:.3e},")
    print("}")
    idx, W, Yt, Y0 = layout_case("rand")
    print("MEASURED_RATES = {")
    for rate in RATES:
        kw = rate_kw(rate)
        dev = float(np.abs(tn.layout(idx, W, Yt, Y0, LAYOUT_EPOCHS, dtype=np.float32, **kw).astype(np.float64)
                           - tn.layout(idx, W, Yt, Y0, LAYOUT_EPOCHS, dtype=np.float64, **kw)).max())
        print(f"    {rate}: {dev:.3e},")
    print("}")
    print("MEASURED_EXACT = {      # case: (cells compared, |port f32 - port f64|)")
    for case in exact_cases():
        f32 = exact_port(*case, np.float32)
        print(f"    {case!r}: ({len(f32)}, {float(np.abs(f32.astype(np.float64) - exact_port(*case, np.float64)).max()):.3e}),")
    print("}")
    cells_tr, lab_tr, cells_te, lab_te, _, _ = holdout()
    nn_idx, nn_dist = un.exact_knn(cells_tr, 15)
    print("MEASURED_QUALITY = [        # (share at the initial positions, share after the sweeps) per seed, by the port")
    for s in QUALITY_SEEDS:
        Ytr, _ = un.umap(nn_idx, nn_dist, umap_init("pca", cells_tr, len(cells_tr), s), QUALITY_EPOCHS, seed=s)
        qi, qd = tn.query_knn(cells_tr, cells_te, 15)
        _, _, W = tn.memberships(qd)
        before = tn.init_positions(qi, W, Ytr)
        after = tn.layout(qi, W, Ytr, before, max(1, round(QUALITY_EPOCHS / 3)), learning_rate=0.25, seed=s)
        print(f"    ({share(Ytr, lab_tr, before, lab_te):.4f}, {share(Ytr, lab_tr, after, lab_te):.4f}),")
    print("]")
    for k in (1, 7, 15):
        qi, _ = tn.query_knn(cells_tr, cells_te, k)
        print(f"brute-force kNN vote, k = {k}: share right = {float((tn.vote(qi, lab_tr) == lab_te).mean()):.4f}")


if __name__ == "__main__":
    _main()
