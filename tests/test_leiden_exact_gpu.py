"""Leiden on the device against the exact restatement of its parallel form, bit for bit (include/gficf_leiden.h: "a function of the
arguments, bit for bit"; gficf_amd/csrc/leiden.hip).

tests/test_leiden_gpu.py compares with a SEQUENTIAL Leiden of another visiting order and so can only bound Q from below.  Here the
yardstick is tests/helpers/leiden_par.py: the header's parallel form — four hash classes, the stamp rule, the refinement's conflict
rule, aggregation in label order — on Python integers, no code shared with the kernels.  Labels, cluster count and the per-level
trace (GFICF_LEIDEN_DEBUG) must be EQUAL, the modularity within 1e-12 of the exact Q rounded once (the device's f64 Q: a u64 over
2W, and sum K^2 over at most n + 1024 doubles, n 2^-53 relative).

Every input is QUALIFIED: the restatement counts no decision on it that f64 could legitimately take the other way
(tests/test_leiden_par_cpu.py asserts that without a device, for every seed and resolution used here; the starts that only a device
can make are asserted here, before the comparison).  Inputs that do not qualify — exact-tie oscillation of local moving to the pass
cap, DESIGN.md §15 — are left out openly: knn_noise_alg2 at seed 1, leiden_cases.hub_graph().

The kernels are chosen by a row's LENGTH at level 0 (wave: up to 128 entries; workgroup beyond, in ceil(min(len, n) / 1024) passes),
so tests/helpers/louvain_forms.cut_rows moves rows between them without changing the graph: every form must give the uncut matrix's
bits.  Every such test asserts from the indptr it sends how many rows take each path."""
import re

import numpy as np
import pytest
import torch

import gficf_amd
from tests.helpers import leiden_cases, leiden_par
from tests.helpers import louvain_forms as lf

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
Q_ABS = 1e-12
GOLDEN = ["knn_blobs", "knn_noise_alg2", "planted3", "planted8_res08"]
WHOLE = [n for n in leiden_cases.EXACT_NAMES if not n.startswith("small")]


@pytest.fixture(scope="module")
def ops():
    return gficf_amd.HipOps(0)


def upload(form):
    indptr, indices, x = form
    return (torch.from_numpy(np.ascontiguousarray(indptr, dtype=np.int64)).to(DEV), torch.from_numpy(np.ascontiguousarray(indices, dtype=np.int32)).to(DEV),
            torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(DEV))


def resident(ops, N, dev, res, n_iterations, seed=0, init=None):
    """(labels, n_clusters, modularity) of HipOps.leiden on rows as they are; the labels start as -7."""
    ws = torch.zeros(ops.leiden_workspace_bytes(N, dev[1].numel()), dtype=torch.uint8, device=DEV)
    lab = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    start = None if init is None else torch.from_numpy(np.ascontiguousarray(init, dtype=np.int32)).to(DEV)
    nc, q = ops.leiden(N, *dev, res, n_iterations, lab, ws, seed, start)
    return lab.cpu().numpy(), nc, q


def resident_refine(ops, N, dev, res, P):
    ws = torch.zeros(ops.leiden_workspace_bytes(N, dev[1].numel()), dtype=torch.uint8, device=DEV)
    out = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    n_ref = ops.leiden_refine(N, *dev, res, torch.from_numpy(np.ascontiguousarray(P, dtype=np.int32)).to(DEV), out, ws)
    return out.cpu().numpy(), n_ref


def hosted(A, res, n_iterations, seed=0, init=None):
    lab = gficf_amd.leiden(A, res, n_iterations, seed, init)
    return np.asarray(lab), lab.n_clusters, lab.modularity


def assert_restated(got, want, what):
    """The device's (labels, n_clusters, modularity) against the restatement's (labels, n_clusters, exact Q)."""
    differ = int((got[0] != want[0]).sum())
    print(what, "clusters", got[1], want[1], "Q", repr(got[2]), repr(want[2]), "labels that differ", differ)
    assert got[0].dtype == np.int32 and got[1] == want[1] and np.array_equal(got[0], want[0]), (what, got[1], want[1], differ)
    assert abs(got[2] - want[2]) < Q_ABS, (what, got[2], want[2])


def assert_same_bits(got, want, what):
    differ = int((got[0] != want[0]).sum())
    print(what, "clusters", got[1], want[1], "Q", repr(got[2]), repr(want[2]), "labels that differ", differ)
    assert got[1] == want[1] and got[2] == want[2] and np.array_equal(got[0], want[0]), (what, got[1], want[1], got[2], want[2], differ)


# ---- the whole run
@pytest.mark.parametrize("name", WHOLE)
def test_whole_run(ops, name):
    A, res = leiden_cases.exact_inputs()[name]
    dev = upload(lf.canonical(A))
    for seed in leiden_cases.exact_seeds(name):
        run = leiden_cases.exact_run(name, seed)
        assert run.fragile == 0
        for n_iterations in (1, 2):
            want = run.after[n_iterations - 1]
            host = hosted(A, res, n_iterations, seed)
            assert_restated(host, want, (name, seed, n_iterations, "host arrays"))
            assert_same_bits(resident(ops, A.shape[0], dev, res, n_iterations, seed), host, (name, seed, n_iterations, "resident tensors"))


@pytest.mark.parametrize("name", ["knn_noise_alg2", "knn_blobs"])
def test_whole_run_from_a_start(ops, name):
    """init = the Louvain partition of the device (as test_leiden_gpu.test_refinement_invariants takes it), spelled with other labels too."""
    A, res = leiden_cases.exact_inputs()[name]
    N = A.shape[0]
    P = np.asarray(gficf_amd.run_modularity_clustering(A, 1, res, 1, 1, 10, 0)).astype(np.int32)
    want = leiden_par.leiden(A, res, 2, 0, init=P)
    print(name, "start of", len(np.unique(P)), "communities: fragile", want.fragile, "passes", [t["passes"] for t in want.trace])
    assert want.fragile == 0, "the start does not qualify: the comparison below would prove nothing"
    assert_restated(hosted(A, res, 2, 0, P), (want.labels, want.n_clusters, want.modularity), (name, "init"))
    assert_restated(hosted(A, res, 1, 0, P), want.after[0], (name, "init, one iteration"))
    spelled = ((N - 1) - P).astype(np.int32)                          # the answer does not depend on how the start is spelled
    assert_same_bits(resident(ops, N, upload(lf.canonical(A)), res, 2, 0, spelled), hosted(A, res, 2, 0, P), (name, "init spelled backwards"))


# ---- the trace: a disagreement names its level and stage
LEVEL = re.compile(r"\[leiden\] level (\d+): (\d+) vertices( \(long rows\))?, (\d+) passes of local moving, Q (-?\d+\.\d{9}), (\d+) communities")
REFINED = re.compile(r"\[leiden\]\s+(\d+) refinement rounds, (\d+) refined communities")


def parse_trace(text):
    out = []
    for line in text.splitlines():
        m = LEVEL.search(line)
        if m:
            out.append(dict(level=int(m.group(1)), vertices=int(m.group(2)), passes=int(m.group(4)), communities=int(m.group(6)), q=float(m.group(5)),
                            rounds=None, refined=None, long_rows=m.group(3) is not None))
            continue
        m = REFINED.search(line)
        if m:
            out[-1]["rounds"], out[-1]["refined"] = int(m.group(1)), int(m.group(2))
    return out


def traced(capfd, monkeypatch, call):
    monkeypatch.setenv("GFICF_LEIDEN_DEBUG", "1")
    capfd.readouterr()
    result = call()
    err = capfd.readouterr().err
    monkeypatch.delenv("GFICF_LEIDEN_DEBUG")
    return result, parse_trace(err)


def assert_trace(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        print(what, "record", i, "device", g, "restated", w)
        for stage in ("level", "vertices", "passes", "communities", "rounds", "refined"):      # in the order the stages run
            assert g[stage] == w[stage], (what, "record", i, "level", w["level"], stage, g[stage], w[stage])
        assert abs(g["q"] - w["q"]) < 0.5e-9 + Q_ABS, (what, "record", i, g["q"], w["q"])       # nine digits are printed
    assert len(got) == len(want), (what, len(got), len(want))


@pytest.mark.parametrize("name", leiden_cases.EXACT_NAMES)
def test_trace(name, capfd, monkeypatch):
    A, res = leiden_cases.exact_inputs()[name]
    for seed in leiden_cases.exact_seeds(name):
        run = leiden_cases.exact_run(name, seed)
        got, trace = traced(capfd, monkeypatch, lambda: hosted(A, res, 2, seed))
        assert len(trace) > 0
        assert_trace(trace, run.trace, (name, seed))
        assert_restated(got, run.after[1], (name, seed, "traced"))


# ---- the refinement alone
@pytest.mark.parametrize("name,start", [("knn_noise_alg2", "louvain"), ("knn_noise_alg2", "one community"), ("knn_blobs", "louvain"),
                                        ("knn_blobs", "one community"), ("standin7", "one iteration"), ("ring8x5", "two components"),
                                        ("ring60x10", "two components")])
def test_refinement_alone(ops, name, start):
    A, res = leiden_cases.exact_inputs()[name]
    N = A.shape[0]
    if start == "louvain":
        P = np.asarray(gficf_amd.run_modularity_clustering(A, 1, res, 1, 1, 10, 0))
    elif start == "one community":
        P = np.zeros(N, dtype=np.int32)
    elif start == "one iteration":
        P = leiden_cases.exact_run(name, 0).after[0][0]
    else:
        P = leiden_cases.disconnected_start(*leiden_cases.RINGS[["ring8x5", "ring60x10"].index(name)])[2]
    want, n_ref, rounds, fragile = leiden_par.refine(A, P, res)
    print(name, start, "refined communities", n_ref, "rounds", rounds, "fragile", fragile)
    assert fragile == 0, "the start does not qualify"
    R = gficf_amd.leiden_refine(A, P, res)
    assert R.dtype == np.int32 and np.array_equal(R, want), (name, start, int((R != want).sum()))
    R2, n2 = resident_refine(ops, N, upload(lf.canonical(A)), res, P)
    assert n2 == n_ref and np.array_equal(R2, want)


# ---- the paths: wave and workgroup kernels, one to three passes over a row, bit for bit
def path_forms():
    A, res = leiden_cases.exact_inputs()[leiden_cases.PATH_GRAPH]
    N, S = A.shape[0], leiden_cases.SEAM_ROWS
    seams, target = leiden_cases.seam_form(A, np.random.default_rng(5))
    return A, res, {
        "seams": (seams, {"wave": N - 4 * S, 1: 2 * S, 2: S, 3: S}, {n: S for n in leiden_cases.SEAM_LENGTHS}),
        "all long": (leiden_cases.all_long_form(A, np.random.default_rng(6)), {"wave": 0, 1: N}, {}),
        "shuffled": (lf.form_shuffle(A, np.random.default_rng(7)), {"wave": N}, {}),
    }


@pytest.mark.parametrize("what", ["seams", "all long", "shuffled"])
def test_paths(ops, what, capfd, monkeypatch):
    A, res, forms = path_forms()
    N = A.shape[0]
    form, paths, lengths = forms[what]
    sent = np.diff(form[0])
    assert leiden_cases.ld_path_counts(form[0], N) == paths, leiden_cases.ld_path_counts(form[0], N)
    for n, rows in lengths.items():
        assert int((sent == n).sum()) >= rows, (n, int((sent == n).sum()))
    if what == "seams":
        assert sorted(set(sent[sent > 128].tolist())) == [129, 1024, 1025, 2049] and int((sent == 128).sum()) >= leiden_cases.SEAM_ROWS
    assert (form[2] > 0).all() and lf.same_graph(lf.fixed_point_matrix(*form, N), lf.fixed_point_matrix(*lf.canonical(A), N))
    plain, cut = upload(lf.canonical(A)), upload(form)
    for seed in leiden_cases.exact_seeds(leiden_cases.PATH_GRAPH):
        run = leiden_cases.exact_run(leiden_cases.PATH_GRAPH, seed)
        for n_iterations in (1, 2):
            got = resident(ops, N, cut, res, n_iterations, seed)
            assert_same_bits(got, resident(ops, N, plain, res, n_iterations, seed), (what, seed, n_iterations, "cut == uncut"))
            assert_restated(got, run.after[n_iterations - 1], (what, seed, n_iterations))
    run = leiden_cases.exact_run(leiden_cases.PATH_GRAPH, 0)
    got, trace = traced(capfd, monkeypatch, lambda: resident(ops, N, cut, res, 2, 0))
    assert trace[0]["long_rows"] == (what != "shuffled")                # the workgroup launches ran on level 0
    assert_trace(trace, run.trace, (what, "trace"))
    for P in (run.after[0][0], np.zeros(N, dtype=np.int32)):
        want, n_ref, _, fragile = leiden_par.refine(A, P, res)
        assert fragile == 0
        R, n2 = resident_refine(ops, N, cut, res, P)
        R0, n0 = resident_refine(ops, N, plain, res, P)
        assert n2 == n0 == n_ref and np.array_equal(R, R0) and np.array_equal(R, want), (what, "refine", int((R != want).sum()))


# ---- scaling: a power of two passes exactly through the fixed point, r, every gain and Q; the bound of the u64 sums
def test_scaling_and_the_fixed_point_bound():
    A, res = leiden_cases.exact_inputs()["planted3"]
    want = hosted(A, res, 2)
    assert_restated(want, leiden_cases.exact_run("planted3", 0).after[1], "planted3")
    up = A * 2.0 ** 18
    assert up.data.max() < 2.0 ** 20 and up.data.max() * lf.SCALE * A.nnz < 9.0e18
    assert_same_bits(hosted(up, res, 2), want, "planted3 x 2^18")
    over = A * 2.0 ** 19
    assert over.data.max() < 2.0 ** 20 and over.data.max() * lf.SCALE * A.nnz >= 9.0e18
    with pytest.raises(gficf_amd.GficfError, match="fixed-point"):
        gficf_amd.leiden(over, res, 2)
    ring, clique = leiden_cases.ring(8, 5)
    top = ring * 2.0 ** 20
    assert top.nnz <= 1998 and top.data.max() == 2.0 ** 20 == top.data.min()
    assert_same_bits(hosted(top, 0.8, 2), hosted(ring, 0.8, 2), "ring x 2^20")
    assert_restated(hosted(top, 0.8, 2), leiden_cases.exact_run("ring8x5", 0).after[1], "ring x 2^20")
    bad = top.copy()
    bad.data[7] = np.nextafter(2.0 ** 20, np.inf)
    with pytest.raises(gficf_amd.GficfError, match=r"outside \[0, 2\^20\]") as e:
        gficf_amd.leiden(bad, 0.8, 2)
    assert "BAD_VALUE" in str(e.value)


# ---- a stored zero is no edge, the diagonal is ignored: neither changes a bit
@pytest.mark.parametrize("name", [f"small{s}" for s in leiden_cases.ZERO_SEEDS] + GOLDEN)
def test_stored_zeros_and_diagonal(ops, name):
    """tests/test_leiden_par_cpu.py shows that on the small graphs a mover that stamped the targets of stored zeros or of the stored
    diagonal would give other labels: k_ld_apply stamps only through entries of non-zero weight."""
    A, res = leiden_cases.exact_inputs()[name]
    N = A.shape[0]
    plain = hosted(A, res, 2)
    assert_restated(plain, leiden_cases.exact_run(name, 0).after[1], (name, "plain"))
    P = plain[0]
    R = gficf_amd.leiden_refine(A, P, res)
    for what, B in (("8 stored zeros a row", leiden_cases.with_stored_zeros(A)), ("a stored diagonal of 0.5", leiden_cases.with_diagonal(A))):
        assert B.nnz > A.nnz and (B != A).nnz == (N if "diagonal" in what else 0)
        assert_same_bits(hosted(B, res, 2), plain, (name, what))
        assert_same_bits(resident(ops, N, upload(lf.canonical(B)), res, 2), plain, (name, what, "resident"))
        assert np.array_equal(gficf_amd.leiden_refine(B, P, res), R), (name, what, "refine")
