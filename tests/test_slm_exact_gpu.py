"""SLM on the device against the exact restatement of its parallel form, bit for bit (include/gficf_slm.h; gficf_amd/csrc/slm.hip).

The yardstick is tests/helpers/slm_par.py: tests/helpers/leiden_par.py's local moving, aggregation and numbering with the fenced
sub-moving in the middle, on Python integers.  Labels, cluster count, iterations and the per-level trace (GFICF_SLM_DEBUG) must be
EQUAL, the modularity within 1e-12 of the exact Q rounded once.  Every input is QUALIFIED (tests/helpers/slm_cases.QUALIFIED,
asserted without a device by tests/test_slm_par_cpu.py); the starts that only a device can make are asserted here first.

The fenced kernels are chosen by a row's LENGTH like the unfenced ones (wave: up to 128 entries; workgroup beyond, in
ceil(min(len, n) / 1024) passes): the seam forms of tests/test_leiden_exact_gpu.py put a partly fenced row at every length."""
import re

import numpy as np
import pytest
import torch

import gficf_amd
from tests.helpers import leiden_cases, slm_cases, slm_par
from tests.helpers import louvain_forms as lf

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
Q_ABS = 1e-12
NAMES = sorted({n for n, _ in slm_cases.QUALIFIED})


@pytest.fixture(scope="module")
def ops():
    return gficf_amd.HipOps(0)


def upload(form):
    indptr, indices, x = form
    return (torch.from_numpy(np.ascontiguousarray(indptr, dtype=np.int64)).to(DEV), torch.from_numpy(np.ascontiguousarray(indices, dtype=np.int32)).to(DEV),
            torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(DEV))


def resident(ops, N, dev, res, n_start, n_iter, seed=0, init=None):
    """(labels, n_clusters, modularity, start, iterations) of HipOps.slm on rows as they are; the labels start as -7."""
    ws = torch.zeros(ops.slm_workspace_bytes(N, dev[1].numel()), dtype=torch.uint8, device=DEV)
    lab = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    start = None if init is None else torch.from_numpy(np.ascontiguousarray(init, dtype=np.int32)).to(DEV)
    nc, q, s, it = ops.slm(N, *dev, res, n_start, n_iter, lab, ws, seed, start)
    return lab.cpu().numpy(), nc, q, s, it


def resident_submove(ops, N, dev, res, P, seed=0, level=0):
    ws = torch.zeros(ops.slm_workspace_bytes(N, dev[1].numel()), dtype=torch.uint8, device=DEV)
    out = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    n_sub, passes = ops.slm_submove(N, *dev, res, torch.from_numpy(np.ascontiguousarray(P, dtype=np.int32)).to(DEV), out, ws, seed, level)
    return out.cpu().numpy(), n_sub, passes


def hosted(A, res, n_start, n_iter, seed=0, init=None):
    lab = gficf_amd.slm(A, res, n_start, n_iter, seed, init)
    return np.asarray(lab), lab.n_clusters, lab.modularity, lab.start, lab.iterations


def assert_restated(got, run, what):
    differ = int((got[0] != run.labels).sum())
    print(what, "clusters", got[1], run.n_clusters, "Q", repr(got[2]), repr(run.modularity), "iterations", got[4], run.iterations, "labels that differ", differ)
    assert got[0].dtype == np.int32 and got[1] == run.n_clusters and np.array_equal(got[0], run.labels), (what, got[1], run.n_clusters, differ)
    assert abs(got[2] - run.modularity) < Q_ABS, (what, got[2], run.modularity)
    assert got[3] == run.start and got[4] == run.iterations, (what, got[3:], run.start, run.iterations)


def assert_same_bits(got, want, what):
    assert got[1:] == want[1:] and np.array_equal(got[0], want[0]), (what, got[1:], want[1:], int((got[0] != want[0]).sum()))


# ---- the trace: a disagreement names its level and stage
LINE = re.compile(r"\[slm\] start=(\d+) iter=(\d+) level=(\d+) vertices=(\d+) long=([01]) passes=(\d+) q=(-?\d+\.\d{9}) communities=(\d+) "
                  r"sub_passes=(-?\d+) sub=(-?\d+)")


def parse_trace(text):
    return [dict(start=int(m[1]), iter=int(m[2]), level=int(m[3]), vertices=int(m[4]), long_rows=m[5] == "1", passes=int(m[6]), q=float(m[7]),
                 communities=int(m[8]), sub_passes=int(m[9]), sub=int(m[10])) for m in LINE.finditer(text)]


def traced(capfd, monkeypatch, call):
    monkeypatch.setenv("GFICF_SLM_DEBUG", "1")
    capfd.readouterr()
    result = call()
    err = capfd.readouterr().err
    monkeypatch.delenv("GFICF_SLM_DEBUG")
    return result, parse_trace(err)


def assert_trace(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        print(what, "record", i, "device", g, "restated", w)
        for stage in ("level", "vertices", "passes", "communities", "sub_passes", "sub"):        # in the order the stages run
            assert g[stage] == w[stage], (what, "record", i, "level", w["level"], stage, g[stage], w[stage])
        assert abs(g["q"] - w["q"]) < 0.5e-9 + Q_ABS, (what, "record", i, g["q"], w["q"])          # nine digits are printed
    assert len(got) == len(want), (what, len(got), len(want))


# ---- the whole run
@pytest.mark.parametrize("name", NAMES)
def test_whole_run(ops, name, capfd, monkeypatch):
    A, res = leiden_cases.exact_inputs()[name]
    dev = upload(lf.canonical(A))
    for seed in [s for n, s in slm_cases.QUALIFIED if n == name]:
        run = slm_cases.exact_run(name, seed)
        assert run.fragile == 0 and run.exact_tie_cap == 0
        host, trace = traced(capfd, monkeypatch, lambda: hosted(A, res, 1, slm_cases.N_ITER, seed))
        assert len(trace) > 0
        assert_trace(trace, run.trace, (name, seed))
        assert_restated(host, run, (name, seed, "host arrays"))
        assert_same_bits(resident(ops, A.shape[0], dev, res, 1, slm_cases.N_ITER, seed), host, (name, seed, "resident tensors"))


# ---- the sub-moving alone
@pytest.mark.parametrize("name,start", [("standin7", "louvain"), ("standin7", "one community"), ("ring8x5", "two components"),
                                        ("standin7", "singletons")])
def test_submoving_alone(ops, name, start):
    A, res = leiden_cases.exact_inputs()[name]
    N = A.shape[0]
    if start == "louvain":
        P = np.asarray(gficf_amd.run_modularity_clustering(A, 1, res, 1, 1, 10, 0)).astype(np.int32)
    elif start == "one community":
        P = np.zeros(N, dtype=np.int32)
    elif start == "singletons":
        P = np.arange(N, dtype=np.int32)[::-1].copy()               # every vertex is its own fence
    else:
        P = leiden_cases.disconnected_start(8, 5)[2]
    for seed, level in ((0, 0), (1234, 2)):
        want, n_sub, passes, fragile = slm_par.submove(A, P, res, seed, level)
        print(name, start, seed, level, "sub-communities", n_sub, "passes", passes, "fragile", fragile)
        assert fragile == 0, "the start does not qualify"
        got = gficf_amd.slm_submove(A, P, res, seed, level)
        assert got.dtype == np.int32 and np.array_equal(got, want), (name, start, int((np.asarray(got) != want).sum()))
        assert got.n_clusters == n_sub and got.passes == passes
        got2, n2, p2 = resident_submove(ops, N, upload(lf.canonical(A)), res, P, seed, level)
        assert n2 == n_sub and p2 == passes and np.array_equal(got2, want)
        assert len(set(zip(want.tolist(), P.tolist()))) == n_sub                                 # inside the fence
        if start == "singletons":
            assert n_sub == N and np.array_equal(got, np.arange(N))
        if start == "two components":
            assert n_sub == 8                                         # the community of two cliques comes apart


# ---- the fenced kernels at every row length
@pytest.mark.parametrize("what", ["seams", "all long"])
def test_fenced_paths(ops, what):
    A, res = leiden_cases.exact_inputs()[leiden_cases.PATH_GRAPH]
    N, S = A.shape[0], leiden_cases.SEAM_ROWS
    if what == "seams":
        form, paths = leiden_cases.seam_form(A, np.random.default_rng(5))[0], {"wave": N - 4 * S, 1: 2 * S, 2: S, 3: S}
    else:
        form, paths = leiden_cases.all_long_form(A, np.random.default_rng(6)), {"wave": 0, 1: N}
    assert leiden_cases.ld_path_counts(form[0], N) == paths
    sent = np.diff(form[0])
    if what == "seams":
        assert sorted(set(sent[sent > 128].tolist())) == [129, 1024, 1025, 2049] and int((sent == 128).sum()) >= S
    assert lf.same_graph(lf.fixed_point_matrix(*form, N), lf.fixed_point_matrix(*lf.canonical(A), N))
    P = slm_cases.three_communities(A, form[0], form[1])            # every row of 128 entries or more lies on both sides of the fence
    want, n_sub, passes, fragile = slm_par.submove(A, P, res)
    assert fragile == 0 and len(np.unique(P)) == 3
    cut, plain = upload(form), upload(lf.canonical(A))
    got, n2, p2 = resident_submove(ops, N, cut, res, P)
    got0, n0, p0 = resident_submove(ops, N, plain, res, P)
    print(what, "sub-communities", n2, n0, n_sub, "passes", p2, p0, passes, "differ", int((got != want).sum()), int((got0 != want).sum()))
    assert n2 == n0 == n_sub and p2 == p0 == passes and np.array_equal(got, got0) and np.array_equal(got, want)
    # and the whole run through the cut rows gives the uncut matrix's bits
    name, seed = "standin7", 4
    run = slm_cases.exact_run(name, seed)
    whole = resident(ops, N, cut, res, 1, slm_cases.N_ITER, seed)
    assert_same_bits(whole, resident(ops, N, plain, res, 1, slm_cases.N_ITER, seed), (what, "cut == uncut"))
    assert_restated(whole, run, (what, "whole run"))


# ---- a stored zero is no edge, the diagonal is ignored: neither changes a bit
def test_stored_zeros_and_diagonal(ops):
    name, seed = "planted8_res08", 0
    A, res = leiden_cases.exact_inputs()[name]
    N = A.shape[0]
    plain = hosted(A, res, 1, slm_cases.N_ITER, seed)
    assert_restated(plain, slm_cases.exact_run(name, seed), (name, "plain"))
    P = plain[0]
    S = gficf_amd.slm_submove(A, P, res)
    for what, B in (("8 stored zeros a row", leiden_cases.with_stored_zeros(A)), ("a stored diagonal of 0.5", leiden_cases.with_diagonal(A))):
        assert B.nnz > A.nnz and (B != A).nnz == (N if "diagonal" in what else 0)
        assert_same_bits(hosted(B, res, 1, slm_cases.N_ITER, seed), plain, (name, what))
        assert_same_bits(resident(ops, N, upload(lf.canonical(B)), res, 1, slm_cases.N_ITER, seed), plain, (name, what, "resident"))
        assert np.array_equal(gficf_amd.slm_submove(B, P, res), S), (name, what, "submove")
