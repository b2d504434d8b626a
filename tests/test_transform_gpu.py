"""GPU: libgficf_transform.so (rectangular search, memberships, initial positions, one-launch layout, vote) and its Python mirror
(find_nn_query, umap_transform, knn_classify, embedNewCells, classify_cells).

Search.  Bit for bit, idx and dist, against the library's own square search (find_nn) wherever that can answer — the training
rows as queries, and distinct queries smuggled in as extra points of a concatenated set — and against counting on a line.

Memberships and initial positions.  Checked against their defining properties in f64 from the device's own sigma, rho and
memberships (tests/helpers/transform_cases.check_memberships): no second implementation in the loop.

Layout against the port, the same table, memberships and initial positions given to both.  The yardstick is the numpy port of
tests/helpers/transform_np.py run in f64.  On every case the port was also run in f32 on the CPU and the largest coordinate
deviation between its two runs recorded: MEASURED below (``python -m tests.helpers.transform_cases`` prints the tables).  The
test constant is 8 x it, never below 64 * 2^-24 * 10 (64 f32 roundings at the largest coordinate).  No row is excluded.  In epoch
0 no entry is due, so the cases over [0, 1) also assert that the coordinates come back untouched.  The cases run at the
transform's default learning rate, 0.25.

Hold-out.  The share of a new cell's 15 nearest trained cells in the plane that carry its label, against the port's own figures
over the same seeds (MEASURED_QUALITY): the blobs separate so well that the port places every new cell among its own, before
and after the sweeps, so this check is loose on purpose; the comparison with the port above is what pins the layout."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import gficf_amd
from gficf_amd import GficfError, synth
from tests.helpers import transform_cases as tc
from tests.helpers import transform_np as tn
from tests.helpers import umap_cases as uc

pytestmark = pytest.mark.gpu

# |port f32 - port f64|, largest coordinate, per layout case (input, curve, epochs of 67), learning rate 0.25
MEASURED = {
    ("rand", "tumap", "0-1"): 0.000e+00,
    ("rand", "tumap", "30-31"): 2.522e-04,
    ("rand", "tumap", "0-3"): 6.540e-05,
    ("rand", "umap", "0-1"): 0.000e+00,
    ("rand", "umap", "30-31"): 7.647e-06,
    ("rand", "umap", "0-3"): 5.230e-05,
    ("crafted", "tumap", "30-31"): 2.522e-04,
}
# the same for epochs [30, 32) at negative_sample_rate = key, seed 3
MEASURED_RATES = {0: 1.150e-06, 1: 1.050e-05, 8: 1.065e-04, 9: 1.306e-04, 20: 4.429e-04}
# (share at the initial positions, share after the sweeps) of the port, seeds 1 - 5: 1 000 blobs cells trained for 200 epochs by the
# port of tests/helpers/umap_np.py, 200 held out and embedded with 67 epochs
MEASURED_QUALITY = [(1.0, 1.0), (1.0, 1.0), (1.0, 1.0), (1.0, 1.0), (1.0, 1.0)]

METRICS = ("manhattan", "euclidean", "cosine", "correlation")


def _same(a, b):
    return np.array_equal(a["idx"], b["idx"]) and np.array_equal(a["dist"].view(np.uint64), b["dist"].view(np.uint64))


# ------------------------------------------------------------------------------------------------ search
@functools.lru_cache(maxsize=None)
def _points(n, d, seed=0):
    return np.random.default_rng(seed).standard_normal((n, d))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d,k", [(1, 1), (2, 15), (5, 16), (50, 17), (50, 64), (50, 65), (128, 128)])
def test_search_with_the_training_rows_as_queries_is_find_nn(d, k, metric):
    X = _points(3000, d)
    assert _same(gficf_amd.find_nn_query(X, X, k, metric), gficf_amd.find_nn(X, k, True, metric))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("k", [1, 15, 88])
def test_search_distinct_queries_against_the_square_search_of_the_concatenation(k, metric):
    """At most 40 of a query's k + 40 nearest points of [X; chunk] are queries, so the first k training ids among them are the
    answer, ties in the same order.  N and M are no multiples of the tiles (128 candidates, 64 queries)."""
    N, M, d = 128 * 7 + 3, 333, 12
    X, Q = _points(N, d, 1), _points(M, d, 2)
    got = gficf_amd.find_nn_query(X, Q, k, metric)
    assert got["idx"].shape == (M, k) and got["idx"].dtype == np.int32 and got["idx"].min() >= 1 and got["idx"].max() <= N
    for lo in range(0, M, 40):
        chunk = Q[lo:lo + 40]
        r = gficf_amd.find_nn(np.concatenate([X, chunk]), k + 40, True, metric)
        for t in range(len(chunk)):
            keep = np.flatnonzero(r["idx"][N + t] <= N)[:k]
            assert np.array_equal(got["idx"][lo + t], r["idx"][N + t][keep]), (lo, t)
            assert np.array_equal(got["dist"][lo + t].view(np.uint64), r["dist"][N + t][keep].view(np.uint64)), (lo, t)


def _line_expected(t, N, k):
    """The k nearest of x_j = j to the query t + 0.25, by counting: t, t + 1, t - 1, t + 2, ... (no ties), 1-based ids."""
    out, step = [], 0
    while len(out) < k:
        cand = [t] if step == 0 else [t + step, t - step]           # distances step - 0.25 < step + 0.25
        out += [j for j in cand if 0 <= j < N]
        step += 1
    out = out[:k]
    return np.array(out) + 1, np.abs(t + 0.25 - np.array(out, dtype=np.float64))


@pytest.mark.parametrize("M", [1, 5])
def test_search_closed_form_on_a_line_with_a_large_split(M):
    N, k = 20000, 15
    ops = tc._ops()
    S = ops.transform_search_split(M, N)
    assert S > 16                                                                    # far beyond the square search's 16 slices
    assert ops.transform_workspace_bytes("search", M, N, k) >= M * S * k * 8
    n_ct = -(-N // 128)
    boundary = (n_ct * (S // 2) // S) * 128                                          # the first point of slice S / 2
    ts = [0, 127, 128, boundary, N - 1][:M] if M == 5 else [boundary]
    X = np.arange(N, dtype=np.float64)[:, None]
    Q = np.array(ts, dtype=np.float64)[:, None] + 0.25
    got = gficf_amd.find_nn_query(X, Q, k, "euclidean")
    for i, t in enumerate(ts):
        ids, dist = _line_expected(t, N, k)
        assert np.array_equal(got["idx"][i], ids), (t, got["idx"][i], ids)
        assert np.array_equal(got["dist"][i], dist), t                               # quarters up to 20 000.25: exact in f32
    man = gficf_amd.find_nn_query(X, Q, k, "manhattan")
    assert _same(man, got)


def test_search_ties_go_to_the_smaller_id():
    rng = np.random.default_rng(3)
    same = np.tile(rng.standard_normal((1, 6)), (20, 1))
    q = rng.standard_normal((1, 6))
    for metric in METRICS:
        r = gficf_amd.find_nn_query(same, q, 20, metric)
        assert np.array_equal(r["idx"][0], np.arange(1, 21)) and np.ptp(r["dist"][0]) == 0, metric
    X = _points(50, 6, 4)
    r = gficf_amd.find_nn_query(X, X[[7, 30]], 3, "euclidean")
    assert r["idx"][:, 0].tolist() == [8, 31] and (r["dist"][:, 0] == 0).all() and (r["dist"][:, 1] > 0).all()
    dup = np.concatenate([X, X[[7]]])                                                # ids 8 and 51 are the same point
    assert gficf_amd.find_nn_query(dup, X[[7]], 2, "euclidean")["idx"][0].tolist() == [8, 51]


def test_search_errors_and_the_context_afterwards():
    X = _points(50, 6, 4)
    bad = X[:5].copy()
    bad[2, 3] = np.nan
    with pytest.raises(GficfError) as e:
        gficf_amd.find_nn_query(X, bad, 3)
    assert e.value.status == "GFICF_ERR_BAD_VALUE"
    for k in (0, 51, 129):
        with pytest.raises(GficfError) as e:
            gficf_amd.find_nn_query(X, X[:5], k)
        assert e.value.status == "GFICF_ERR_INVALID_ARG", k
    with pytest.raises(ValueError):
        gficf_amd.find_nn_query(X, X[:5, :4], 3)
    r = gficf_amd.find_nn_query(X, X[:5], 3)                                         # the context is still good
    assert r["idx"][:, 0].tolist() == [1, 2, 3, 4, 5]
    assert gficf_amd.find_nn_query(X, X[:0], 3)["idx"].shape == (0, 3)               # no queries: nothing to do


# ------------------------------------------------------------------------------------------------ memberships and init
@pytest.mark.parametrize("k", tc.MEMBERSHIP_KS)
@pytest.mark.parametrize("lc", tc.MEMBERSHIP_LCS)
def test_memberships_properties(k, lc):
    idx, dist, N = tc.membership_table(k)
    W, sigma, rho = tc.dev_weights(idx, dist, N, lc)
    tc.check_memberships(dist, sigma, rho, W, lc)
    if lc == 1.0:
        assert (rho == 0).all()
    assert (W[tc.ROW_ZERO] == 1).all() and np.ptp(W[tc.ROW_EQUAL]) == 0
    W2, sigma2, rho2 = tc.dev_weights(idx, dist, N, lc)
    assert np.array_equal(W, W2) and np.array_equal(sigma, sigma2) and np.array_equal(rho, rho2)


def test_memberships_deferred_errors():
    idx, dist, N = tc.membership_table(15)
    for v in (0, N + 1):
        bad = idx.copy()
        bad[7, 2] = v
        with pytest.raises(GficfError) as e:
            tc.dev_weights(bad, dist, N)
        assert e.value.status == "GFICF_ERR_BAD_ID"
    for v in (np.nan, np.inf):
        d = dist.copy()
        d[9, 3] = v
        with pytest.raises(GficfError) as e:
            tc.dev_weights(idx, d, N)
        assert e.value.status == "GFICF_ERR_BAD_VALUE"
    d = dist.copy()
    d[:, 0] = -1e-7                                                                  # what 1 - cos rounds to: taken as 0
    d0 = dist.copy()
    d0[:, 0] = 0.0
    assert np.array_equal(tc.dev_weights(idx, d, N)[0], tc.dev_weights(idx, d0, N)[0])
    with pytest.raises(GficfError) as e:
        tc.dev_weights(idx, dist, N, lc=0.5)
    assert e.value.status == "GFICF_ERR_INVALID_ARG"


@pytest.mark.parametrize("k", tc.MEMBERSHIP_KS)
def test_init_against_f64_from_the_devices_own_memberships(k):
    idx, dist, N = tc.membership_table(k)
    Yt = (np.random.default_rng(k).uniform(-10, 10, size=(N, 2))).astype(np.float32)
    W, _, _ = tc.dev_weights(idx, dist, N)
    W[3] = 0.0                                                                       # no membership at all: the plain mean
    Y0 = tc.dev_init(idx, W, Yt)
    w64, y64 = W.astype(np.float64), Yt.astype(np.float64)[idx - 1]
    with np.errstate(invalid="ignore"):
        want = (w64[:, :, None] * y64).sum(1) / w64.sum(1)[:, None]
    want[3] = y64[3].mean(0)
    tol = 2 * (k + 2) * 2.0 ** -24 * float(np.abs(Yt).max())                         # k adds above, k below, one division
    err = float(np.abs(Y0.astype(np.float64) - want).max())
    print(f"k = {k}: |device - f64| = {err:.3e}, tolerance {tol:.3e}")
    assert Y0.dtype == np.float32 and np.isfinite(Y0).all() and err <= tol
    bad = Yt.copy()
    bad[N - 1, 1] = np.inf                                                           # a trained cell nobody may name
    with pytest.raises(GficfError) as e:
        tc.dev_init(idx, W, bad)
    assert e.value.status == "GFICF_ERR_BAD_VALUE"


# ------------------------------------------------------------------------------------------------ layout against the port
@pytest.mark.parametrize("case", tc.layout_cases(), ids=lambda c: "-".join(c))
def test_layout_against_port(case):
    got, Y0 = tc.dev_layout_case(*case)
    want = tc.port_layout(*case, np.float64)
    err = float(np.abs(got.astype(np.float64) - want).max())
    tol = tc.tolerance(MEASURED[case])
    moved = float(np.abs(want - Y0).max())
    print(f"{case}: |device - port f64| = {err:.3e}, port f32 / f64 = {MEASURED[case]:.3e}, tolerance {tol:.3e}, moved {moved:.3e}")
    assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all()
    assert err <= tol
    if case[2] == "0-1":
        assert np.array_equal(got, Y0)                                               # no entry is due in epoch 0
    else:
        assert moved > 10 * tol                                                      # the sweep is far above what the tolerance forgives


def test_layout_crafted_case_takes_the_zero_distance_branch():
    idx, W, Yt, Y0 = tc.layout_case("crafted")
    assert np.array_equal(Y0[tc.CRAFTED], Yt[idx[tc.CRAFTED, 0] - 1])
    lo, _ = tc.RANGES[tc.CRAFTED_EPOCH]
    assert tn.due(tn.row_schedule(W)[tc.CRAFTED, 0], lo).all()                       # an attraction at d2 == 0 happens in that epoch


# ------------------------------------------------------------------------------------------------ layout: bits
@pytest.mark.parametrize("ab", list(tc.AB))
def test_layout_bits(ab):
    idx, W, Yt, Y0 = tc.layout_case("rand")
    a, b = tc.AB[ab]
    run = functools.partial(tc.dev_layout, n_epochs=67, a=a, b=b, learning_rate=0.25)
    whole = run(idx, W, Yt, Y0, seed=7)
    assert np.array_equal(run(idx, W, Yt, Y0, seed=7), whole) and np.isfinite(whole).all()
    first = run(idx, W, Yt, Y0, seed=7, epoch_begin=0, epoch_end=33)
    assert np.array_equal(run(idx, W, Yt, first, seed=7, epoch_begin=33, epoch_end=67), whole)
    lo = run(idx[:250], W[:250], Yt, Y0[:250], seed=7, query_offset=0)
    hi = run(idx[250:], W[250:], Yt, Y0[250:], seed=7, query_offset=250)
    assert np.array_equal(np.concatenate([lo, hi]), whole)
    assert not np.array_equal(run(idx[250:], W[250:], Yt, Y0[250:], seed=7, query_offset=0), whole[250:])
    assert not np.array_equal(run(idx, W, Yt, Y0, seed=8), whole)


@pytest.mark.parametrize("rate", tc.RATES)                                           # fewer than, as many as and more than the lanes of a group
def test_layout_negative_sample_rates(rate):
    idx, W, Yt, Y0 = tc.layout_case("rand")
    kw = tc.rate_kw(rate)
    got = tc.dev_layout(idx, W, Yt, Y0, tc.LAYOUT_EPOCHS, **kw)
    want = tn.layout(idx, W, Yt, Y0, tc.LAYOUT_EPOCHS, dtype=np.float64, **kw)
    err, tol = float(np.abs(got - want).max()), tc.tolerance(MEASURED_RATES[rate])
    print(f"rate {rate}: |device - port f64| = {err:.3e}, port f32 / f64 = {MEASURED_RATES[rate]:.3e}, tolerance {tol:.3e}")
    assert err <= tol


def test_layout_errors():
    idx, W, Yt, Y0 = tc.layout_case("rand")
    bad = Y0.copy()
    bad[17, 1] = np.nan
    with pytest.raises(GficfError) as e:
        tc.dev_layout(idx, W, Yt, bad, 5)
    assert e.value.status == "GFICF_ERR_BAD_VALUE"
    bad_id = idx.copy()
    bad_id[3, 3] = len(Yt) + 1
    with pytest.raises(GficfError) as e:
        tc.dev_layout(bad_id, W, Yt, Y0, 5)
    assert e.value.status == "GFICF_ERR_BAD_ID"
    for kw in (dict(epoch_begin=3, epoch_end=2), dict(query_offset=-1), dict(negative_sample_rate=-1), dict(a=0.0)):
        with pytest.raises(GficfError) as e:
            tc.dev_layout(idx, W, Yt, Y0, 5, **kw)
        assert e.value.status == "GFICF_ERR_INVALID_ARG", kw
    assert np.isfinite(tc.dev_layout(idx, W, Yt, Y0, 5)).all()                       # the context is still good


# ------------------------------------------------------------------------------------------------ chain
def _model(Yt, ab="umap", seed=5):
    a, b = tc.AB[ab]
    return {"embedding": Yt.astype(np.float64), "a": a, "b": b, "n_neighbors": 15, "metric": "euclidean", "n_epochs": 200, "seed": seed}


def test_chain_equals_its_stages():
    """gficf_transform_host against find_nn_query -> memberships -> init -> layout called one by one, bit for bit, and the
    device-resident chain of HipOps (every stage reads the one before's own output, no copy or conversion in between)."""
    X, Q = uc.random_input(1500), uc.random_input(500, seed=6)
    Yt = uc.plane_init(X).astype(np.float32)
    model = _model(Yt)
    r = gficf_amd.umap_transform(Q, model, X, ret_extra=True)
    assert np.array_equal(gficf_amd.umap_transform(Q, model, X), r["embedding"])
    nn = gficf_amd.find_nn_query(X, Q, 15)
    assert np.array_equal(r["idx"], nn["idx"]) and np.array_equal(r["dist"], nn["dist"].astype(np.float32))
    W, sigma, rho = tc.dev_weights(nn["idx"], nn["dist"], len(X))
    assert np.array_equal(r["w"], W) and np.array_equal(r["sigma"], sigma) and np.array_equal(r["rho"], rho)
    Y0 = tc.dev_init(nn["idx"], W, Yt)
    assert np.array_equal(r["init"], Y0.astype(np.float64))
    Y = tc.dev_layout(nn["idx"], W, Yt, Y0, 67, model["a"], model["b"], 1.0, 0.25, 5, 5)
    assert np.array_equal(r["embedding"], Y.astype(np.float64)) and not np.array_equal(Y, Y0)
    given = gficf_amd.umap_transform(Q, model, X, init=Y0, epoch_begin=0, epoch_end=20)      # a given start, part of the sweeps
    rest = gficf_amd.umap_transform(Q, model, X, init=given, epoch_begin=20)
    assert np.array_equal(rest, r["embedding"])
    halves = [gficf_amd.umap_transform(Q[:200], model, X), gficf_amd.umap_transform(Q[200:], model, X, query_offset=200)]
    assert np.array_equal(np.concatenate(halves), r["embedding"])

    import torch

    ops = tc._ops()
    (N, d), M, k, dev = X.shape, len(Q), 15, "cuda:0"
    pts = torch.zeros((N, ops.knn_dpad(d)), dtype=torch.float32, device=dev)
    qry = torch.zeros((M, ops.knn_dpad(d)), dtype=torch.float32, device=dev)
    ops.knn_prepare(torch.from_numpy(np.ascontiguousarray(X.T)).to(dev), N, d, "euclidean", pts)
    ops.knn_prepare(torch.from_numpy(np.ascontiguousarray(Q.T)).to(dev), M, d, "euclidean", qry)
    sws = torch.empty(ops.transform_workspace_bytes("search", M, N, k), dtype=torch.uint8, device=dev)
    d_idx = torch.empty((k, M), dtype=torch.int32, device=dev)
    d_dist = torch.empty((k, M), dtype=torch.float32, device=dev)
    ops.transform_search(pts, N, qry, M, d, k, "euclidean", sws, d_idx, d_dist)
    d_w = torch.empty((k, M), dtype=torch.float32, device=dev)
    wws, iws, lws = (torch.empty(ops.transform_workspace_bytes(s, M, k=k), dtype=torch.uint8, device=dev) for s in ("weights", "init", "layout"))
    ops.transform_weights(d_idx, d_dist, N, M, k, wws, d_w)
    d_Yt = torch.from_numpy(Yt).to(dev)
    d_Y = torch.empty((M, 2), dtype=torch.float32, device=dev)
    ops.transform_init(d_idx, d_w, d_Yt, N, M, k, iws, d_Y)
    ops.transform_layout(d_idx, d_w, d_Yt, N, M, k, model["a"], model["b"], 1.0, 0.25, 5, 67, 0, 67, 5, 0, d_Y, lws)
    for ws in (sws, wws, iws, lws):
        ops.transform_sync(ws)
    assert np.array_equal(d_Y.cpu().numpy(), Y)


# ------------------------------------------------------------------------------------------------ workflow
def test_holdout_cells_land_among_their_own():
    cells_tr, lab_tr, cells_te, lab_te, _, _ = tc.holdout()
    floor = min(after for _, after in MEASURED_QUALITY) - 0.01
    for seed in tc.QUALITY_SEEDS:
        data = gficf_amd.runReduction({"pca": {"cells": cells_tr}}, seed=seed, n_epochs=tc.QUALITY_EPOCHS, verbose=False)
        r = gficf_amd.umap_transform(cells_te, data["uwot"], cells_tr, ret_extra=True)
        Ytr = np.asarray(data["embedded"])
        before, after = tc.share(Ytr, lab_tr, r["init"], lab_te), tc.share(Ytr, lab_tr, r["embedding"], lab_te)
        print(f"seed {seed}: share before the sweeps {before:.4f}, after {after:.4f} (port at least {floor + 0.01:.4f})")
        assert np.isfinite(r["embedding"]).all() and after >= floor


@pytest.mark.parametrize("k", [1, 7, 15])
def test_knn_classify_on_the_holdout(k):
    cells_tr, lab_tr, cells_te, lab_te, _, _ = tc.holdout()
    pred = gficf_amd.knn_classify(cells_tr, cells_te, lab_tr, k)
    assert pred.dtype == lab_tr.dtype and np.array_equal(pred, lab_te)               # brute force on the CPU gets every one right too
    names = np.array([f"type{v:02d}" for v in lab_tr])
    assert np.array_equal(gficf_amd.knn_classify(cells_tr, cells_te, names, k), np.array([f"type{v:02d}" for v in lab_te]))


@pytest.mark.parametrize("C", [2, 12, 300])
@pytest.mark.parametrize("k", [1, 7, 128])
def test_vote_against_numpy(C, k):
    rng = np.random.default_rng(C * 1000 + k)
    M = 200
    T = rng.integers(0, C, size=(M, k)).astype(np.int32)
    a, b = 1, 0
    forced = k >= 7 and (C > 2 or k % 2 == 0)                                        # (two classes and an odd k cannot tie)
    if forced:                                                                       # a and b tie at k // 2 votes: the one met first wins
        tail = [2] * (k % 2)
        T[0] = [a, b] * (k // 2) + tail
        T[1] = [b, a] * (k // 2) + tail
        T[2] = tail + [b, a] * (k // 2)
        T[3] = a
    idx = np.arange(M * k, dtype=np.int32).reshape(M, k) + 1                         # distinct ids: the label table is the rows' labels
    labels = T.ravel()
    pred, votes = tc.dev_vote(idx, labels, C, want_votes=True)
    assert np.array_equal(pred, tn.vote(idx, labels))
    assert np.array_equal(votes, np.stack([np.bincount(row, minlength=C) for row in T]))
    assert np.array_equal(tc.dev_vote(idx, labels, C), pred)
    if forced:
        assert pred[:4].tolist() == [a, b, b, a]
    bad = labels.copy()
    bad[5] = C
    with pytest.raises(GficfError) as e:
        tc.dev_vote(idx, bad, C)
    assert e.value.status == "GFICF_ERR_BAD_ID"


@pytest.fixture(scope="module")
def trained():
    colptr, rowidx, x = synth.counts_csc(1500, 800)
    M = sp.csc_matrix((x, rowidx, colptr), shape=(1500, 800))
    data = gficf_amd.gficf(M[:, :650], normalize=False, verbose=False)
    data = gficf_amd.runPCA(data, dim=10)
    data = gficf_amd.runReduction(data, n_epochs=60, verbose=False)
    data = gficf_amd.clustcells(data, verbose=False)
    return data, M[:, 650:]


def test_embed_and_classify_end_to_end(trained):
    data, new = trained
    before = np.asarray(data["embedded"][["X", "Y"]]).copy()
    new = new.tolil()
    gene = int(data["genes"][3])
    new[gene, :] = 0                                                                 # a kept gene absent from every new cell
    data = gficf_amd.embedNewCells(data, new.tocsc(), verbose=False)
    emb = data["embedded"]
    assert len(emb) == 800 and (emb["predicted"] == "YES").sum() == 150 and (emb["predicted"][:650] == "NO").all()
    assert list(emb["predicted"].cat.categories) == ["NO", "YES"]
    xy = np.asarray(emb[["X", "Y"]])
    assert np.isfinite(xy).all() and np.array_equal(xy[:650].view(np.uint64), before.view(np.uint64))
    assert data["pca"]["pred"].shape == (150, 10) and np.isfinite(data["pca"]["pred"]).all()
    classes = data["cluster"]
    for method in ("PCA", "embedded"):
        df = gficf_amd.classify_cells(data, classes, method=method)
        assert list(df.columns) == ["cell.id", "pred"] and len(df) == 150
        assert set(df["pred"]) <= set(classes) and list(df["cell.id"]) == list(range(650, 800))
    again = gficf_amd.embedNewCells({**data, "embedded": emb.iloc[:650][["X", "Y"]], "pca": dict(data["pca"])}, new.tocsc(), verbose=False,
                                    genes=data["genes"])
    assert np.array_equal(np.asarray(again["embedded"][["X", "Y"]]), xy)             # genes= given; the same bits on a second call
