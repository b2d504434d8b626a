"""Louvain's degree-class kernels against each other, bit for bit (gficf_amd/csrc/louvain.hip).

The local moving and the reduction each have three kernels and five regimes, chosen by a row's LENGTH (k_lv_list_big: end - beg):

    row length               local moving                                    reduction
    <= 64, several starts    k_lv_move_small, two copies per round ("pair")   k_lv_emit_small
    <= 128                   k_lv_move_small, two entries per lane            k_lv_emit_small
    129 .. 512               k_lv_move_mid, one pass                          k_lv_emit_big<2048>
    513 .. 4096              k_lv_move_mid, ceil(len / 512) passes            k_lv_emit_big<2048>, ceil(len / 1024) passes
    > 4096                   k_lv_move_big, ceil(len / 4096) passes           k_lv_emit_big<8192>

All sums are integers in 2^-32 fixed point and every form computes the same function of (labels, totals, sizes, per-community sums), so
two matrices whose rows hold the same per-neighbour fixed-point sums must give the same labels, cluster count and modularity — equal
bits, not close — however the sums are cut into entries and however the entries are ordered (the file's header promises the second; the
coarse rows the reduction builds with atomics rely on it).  tests/helpers/louvain_forms.py cuts and shuffles; tests/test_louvain_forms_cpu.py
shows on the CPU that its forms are the graph they were made from.  The forms go through HipOps.louvain (gficf_louvain_device), which takes
rows as they are; run_modularity_clustering sorts them first.  Every test asserts, from the indptr it sends, how many rows fall into each class,
so a test that stopped reaching a kernel fails: at level 0 the class is a function of the row length alone."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gficf_amd
from gficf_amd.api import ClusterLabels
from oracle import oracle_np
from tests.helpers import louvain_forms as lf
from tests.test_louvain_gpu import check_labels, hub_graph, knn_graph, same_partition

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the parameter grid: (algorithm, n_start, n_iter, resolution, seed)
ONE = dict(algorithm=1, n_start=1, n_iter=10, res=0.8, seed=0)
THREE = dict(algorithm=1, n_start=3, n_iter=10, res=0.8, seed=4242)       # pair rounds in k_lv_move_small, the last copy unpaired; rep > 1 in mid / big
REFINE = dict(algorithm=2, n_start=2, n_iter=10, res=1.0, seed=0)         # the rebuilt levels run k_lv_emit_big on the level-0 rows
FN2 = dict(algorithm=1, n_start=1, n_iter=10, res=0.05, seed=0, function=2)
LINES = {"one": ONE, "three": THREE, "refine": REFINE, "fn2": FN2}
GRID = ("one", "three", "refine")


@pytest.fixture(scope="module")
def ops():
    return gficf_amd.HipOps(0)


def upload(form):
    indptr, indices, x = form
    return torch.from_numpy(indptr).to(DEV), torch.from_numpy(indices).to(DEV), torch.from_numpy(x).to(DEV)


def run(ops, N, indptr, indices, x, res, n_iter, algorithm, n_start, seed, ws_starts=None):
    """(labels, n_clusters, modularity) of HipOps.louvain on rows as they are (numpy arrays or device tensors); the workspace is
    louvain_workspace_bytes(N, nnz, ws_starts or n_start) bytes, the labels start as -7."""
    if isinstance(indptr, np.ndarray):
        indptr, indices, x = upload((indptr, indices, x))
    assert indptr.dtype == torch.int64 and indices.dtype == torch.int32 and x.dtype == torch.float64 and indptr.numel() == N + 1
    ws = torch.zeros(ops.louvain_workspace_bytes(N, indices.numel(), ws_starts or n_start), dtype=torch.uint8, device=DEV)
    lab = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    nc, q = ops.louvain(N, indptr, indices, x, res, n_iter, lab, ws, algorithm, n_start, seed)
    labels = lab.cpu().numpy()
    assert labels.min() >= 0 and labels.max() == nc - 1
    return labels, nc, q


def run_line(ops, N, dev, line):
    p = dict(LINES[line])
    fn = p.pop("function", 1)
    if fn == 1:
        return run(ops, N, *dev, **p)
    ops.L.gficf_ctx_set_louvain_options(ops.ctx.handle, fn)             # as run_modularity_clustering does it
    try:
        return run(ops, N, *dev, **p)
    finally:
        ops.L.gficf_ctx_set_louvain_options(ops.ctx.handle, 1)


def assert_same(got, want, what):
    differ = int((got[0] != want[0]).sum())
    print(what, "clusters", got[1], want[1], "Q", repr(got[2]), repr(want[2]), "labels that differ", differ)
    assert got[1] == want[1] and got[2] == want[2] and np.array_equal(got[0], want[0]), (what, got[1], want[1], got[2], want[2], differ)


def as_cluster_labels(result):
    lab = result[0].view(ClusterLabels)
    lab.n_clusters, lab.modularity = result[1], result[2]
    return lab


# ---- the base graphs (quantised), their canonical form on the device, and the canonical results: made once
_graphs, _canon = {}, {}


def graph(name):
    if name not in _graphs:
        if name == "g1":
            A = knn_graph(3000, 10, 15, 1, seed=101)                      # structureless: many near-ties, labels sensitive to any single decision
        elif name == "g2":
            A = knn_graph(6000, 10, 30, 8, seed=102)                      # clustered
        elif name == "g3":
            A = hub_graph()                                               # hubs of 30 000 and 3 000
        elif name == "g4":
            A = lf.many_hubs_graph()[0]                                   # 200 hubs of 130 .. 9000: hundreds of distinct keys in the multi-pass tables
        elif name == "small":
            A = knn_graph(2000, 10, 15, 1, seed=103)
        Q = lf.quantise(A)
        _graphs[name] = (Q, upload(lf.canonical(Q)))
    return _graphs[name]


def canonical_result(ops, name, line, env=""):
    key = (name, line, env)
    if key not in _canon:
        Q, dev = graph(name)
        _canon[key] = run_line(ops, Q.shape[0], dev, line)
        lab = as_cluster_labels(_canon[key])
        p = LINES[line]
        if p.get("function", 1) == 1:
            check_labels(Q, lab, p["res"])
        else:
            assert abs(lab.modularity - oracle_np.modularity_np(Q, lab, p["res"], 2)) < 1e-9
    return _canon[key]


def assert_classes(indptr, n_start, exactly=None, at_least=None):
    """The rows per class of the indptr that is sent.  The first class is a regime of its own only with several starts (pair rounds)."""
    counts = lf.class_counts(indptr)
    print("rows per class", counts, "passes (move_mid, emit_big<2048>, move_big / emit_big<8192>)", lf.pass_counts(indptr), "n_start", n_start)
    for c, n in (exactly or {}).items():
        assert counts[c] == n, (c, counts)
    for c, n in (at_least or {}).items():
        assert counts[c] >= n, (c, counts)
    return counts


def compare(ops, name, form, lines, exactly=None, at_least=None, env=""):
    """The form against the canonical form of its graph, on every line; the form is first shown to be that graph."""
    Q, _ = graph(name)
    N = Q.shape[0]
    assert lf.same_graph(lf.fixed_point_matrix(*form, N), lf.fixed_point_matrix(*lf.canonical(Q), N))
    dev = upload(form)
    for line in lines:
        assert_classes(form[0], LINES[line]["n_start"], exactly, at_least)
        assert_same(run_line(ops, N, dev, line), canonical_result(ops, name, line, env), (name, line, env))


# ---- form 1: the entry-order promise
@pytest.mark.parametrize("name", ["g1", "g2", "g3", "g4"])
def test_entry_order_does_not_matter(ops, name):
    Q, _ = graph(name)
    N = Q.shape[0]
    exactly = {"g1": {"le64": N}, "g2": {"midP": 0, "big": 0}, "g3": {"le64": N - 2, "midP": 1, "big": 1},
               "g4": {"le64": N - 200, "le128": 0}}[name]
    at_least = {"g2": {"le64": 100, "le128": 100}, "g4": {"mid1": 20, "midP": 20, "big": 10}}.get(name)
    form = lf.form_shuffle(Q, np.random.default_rng(11))
    assert not np.array_equal(form[1], Q.indices)
    compare(ops, name, form, GRID + ("fn2",), exactly, at_least)


# ---- form 2: the raw-array route is the mirror's
@pytest.mark.parametrize("name", ["g1", "g2", "g3", "g4"])
def test_raw_arrays_equal_the_mirror(ops, name):
    Q, _ = graph(name)
    host = gficf_amd.run_modularity_clustering(Q, 1, ONE["res"], 1, 1, 10, 0, False)
    assert_same(canonical_result(ops, name, "one"), (np.asarray(host), host.n_clusters, host.modularity), name)


# ---- form 3: uniform cut factors that put the bulk of the rows into each class
@pytest.mark.parametrize("name,factor,lines,at_least", [
    ("g1", 3, GRID, {"le64": 100, "le128": 100}),                         # straddles 64 and 128
    ("g2", 3, GRID + ("fn2",), {"le128": 100, "mid1": 100}),
    ("g1", 12, GRID + ("fn2",), {"mid1": 1000}),                          # straddles 512
    ("g2", 12, GRID, {"mid1": 100, "midP": 100}),
    ("g1", 90, GRID, {"midP": 1000}),                                     # up to 4096 and beyond: about 8 M entries
])
def test_uniform_cut(ops, name, factor, lines, at_least):
    Q, _ = graph(name)
    form = lf.form_uniform(Q, factor, np.random.default_rng(factor))
    assert np.array_equal(np.diff(form[0]), np.diff(Q.indptr) * factor)
    compare(ops, name, form, lines, None, at_least)


def test_every_row_in_the_workgroup_kernel(ops):
    """x300 on a structureless graph of 2000 vertices (rows of fewer than 14 entries, which x300 leaves at 4096 or below, by as much as takes
    them beyond): every row beyond 4096 entries, k_lv_move_big with 2 to 4 and more passes (about 12 M entries)."""
    Q, _ = graph("small")
    form = lf.form_all_big(Q, 300, np.random.default_rng(300))
    assert np.diff(form[0]).min() > 4096 and len(form[1]) > 10_000_000
    _, _, big_passes = lf.pass_counts(form[0])
    assert big_passes[:3] == [2, 3, 4], big_passes
    compare(ops, "small", form, GRID + ("fn2",), {"big": Q.shape[0]})


# ---- form 4: all classes side by side
def test_mixed_factors(ops, monkeypatch):
    Q, _ = graph("g1")
    form = lf.form_mixed(Q, np.random.default_rng(4))
    every = {c: 20 for c in lf.CLASS_NAMES}
    compare(ops, "g1", form, GRID + ("fn2",), None, every)
    monkeypatch.setenv("GFICF_LOUVAIN_SUBROUNDS", "3")                    # the only class count that is no power of two: lv_class takes its % branch
    compare(ops, "g1", form, ("one", "three"), None, every, env="subrounds3")
    monkeypatch.delenv("GFICF_LOUVAIN_SUBROUNDS")
    assert not np.array_equal(canonical_result(ops, "g1", "one")[0], canonical_result(ops, "g1", "one", "subrounds3")[0])   # the knob was read


# ---- form 5: exact seams
def test_exact_seams(ops):
    Q, _ = graph("g2")
    form, target = lf.form_seams(Q, np.random.default_rng(5))
    got = np.diff(form[0])
    assert np.array_equal(got, np.where(target >= 0, target, np.diff(Q.indptr)))
    for n in lf.SEAM_LENGTHS:
        assert (got[target >= 0] == n).sum() == 40
    compare(ops, "g2", form, ("one", "three"), {"midP": 160, "big": 120}, {"le64": 80, "le128": 80, "mid1": 80})


# ---- form 6: the pass partition changes (and with it the hash class of every community)
@pytest.mark.parametrize("name,n_hubs", [("g3", 2), ("g4", 200)])
@pytest.mark.parametrize("factor", [2, 3])
def test_pass_partition_changes(ops, name, n_hubs, factor):
    Q, _ = graph(name)
    deg = np.diff(Q.indptr)
    form = lf.form_rows(Q, np.arange(n_hubs), factor, np.random.default_rng(60 + factor))
    hub_len = deg[:n_hubs] * factor
    assert np.array_equal(np.diff(form[0])[:n_hubs], hub_len) and np.array_equal(np.diff(form[0])[n_hubs:], deg[n_hubs:])
    before, after = lf.class_counts(Q.indptr), lf.class_counts(form[0])
    assert lf.pass_counts(Q.indptr) != lf.pass_counts(form[0])
    if name == "g3":
        exactly = {"le64": Q.shape[0] - 2, "midP": 0, "big": 2}           # 3000 -> 6000 / 9000 entries: k_lv_move_mid -> k_lv_move_big
    else:
        exactly = {c: int(n) for c, n in zip(lf.CLASS_NAMES[1:], np.bincount(np.searchsorted(lf.CLASS_EDGES, hub_len, side="left"), minlength=5)[1:])}
        assert after["big"] >= before["big"] + 10 and after["mid1"] <= before["mid1"] - 10          # many rows cross 512 and 4096
    lines = GRID + ("fn2",) if (name, factor) in (("g3", 2), ("g4", 3)) else GRID
    compare(ops, name, form, lines, exactly)


# ---- form 7: one vertex in 50 promoted to one class — when a form above fails, this names the kernel
@pytest.mark.parametrize("cls", lf.CLASS_NAMES)
def test_one_vertex_in_fifty_promoted(ops, cls):
    Q, _ = graph("g1")
    N = Q.shape[0]
    form, target = lf.form_promote(Q, cls, np.random.default_rng(70))
    assert ((np.diff(form[0]) == lf.PROMOTE_LENGTHS[cls]) & (target >= 0)).sum() == N // 50
    exactly = {"le64": N} if cls == "le64" else {"le64": N - N // 50, cls: N // 50}
    compare(ops, "g1", form, ("one", "three"), exactly)


# ---- exact properties of the partition (check_labels): components never merge, a vertex without edges stays alone
@pytest.mark.parametrize("n_start", [1, 4])
def test_components_and_isolated_vertices(ops, n_start):
    A, comp = lf.components_graph()
    assert (comp < 0).sum() == 50 and comp.max() == 301
    lab = gficf_amd.run_modularity_clustering(A, 1, 0.8, 1, n_start, 10, 3, False)
    check_labels(A, lab, 0.8)
    lab = np.asarray(lab)
    sizes = np.bincount(lab)
    assert (sizes[lab[comp < 0]] == 1).all()
    inside = comp >= 0
    pairs = np.unique(np.stack([lab[inside], comp[inside]], axis=1), axis=0)
    assert len(pairs) == len(np.unique(lab[inside]))                      # every cluster lies in one component
    assert len(np.unique(lab[inside])) >= 302
    Q = lf.quantise(A)
    form = lf.form_shuffle(Q, np.random.default_rng(9))
    N = Q.shape[0]
    p = dict(algorithm=1, n_start=n_start, n_iter=10, res=0.8, seed=3)
    want = run(ops, N, *lf.canonical(Q), **p)
    check_labels(Q, as_cluster_labels(want), 0.8)
    assert_same(run(ops, N, *form, **p), want, "components, shuffled")


# ---- the result does not depend on how many starts the workspace lets run together
def test_workspace_size_does_not_matter(ops):
    Q, dev = graph("g1")
    N = Q.shape[0]
    mixed = lf.form_mixed(Q, np.random.default_rng(4))
    for what, d, nnz in (("canonical", dev, Q.nnz), ("mixed", upload(mixed), len(mixed[1]))):
        sizes = [ops.louvain_workspace_bytes(N, nnz, s) for s in (1, 2, 5)]
        assert sizes[0] < sizes[1] < sizes[2]
        p = dict(algorithm=1, n_start=5, n_iter=10, res=0.8, seed=4242)
        results = [run(ops, N, *d, ws_starts=s, **p) for s in (1, 2, 5)]
        assert_same(results[0], results[2], (what, "workspace for 1 start"))
        assert_same(results[1], results[2], (what, "workspace for 2 starts"))
    assert_same(results[2], run(ops, N, *dev, **p), "mixed == canonical, 5 starts")


# ---- algorithm 2 keeps the vertex maps of LV_MAX_SAVED = 12 levels: a descent that is deeper
DEEP_CHILD = r"""
import sys
import numpy as np
import gficf_amd
from tests.helpers import louvain_forms as lf
from tests.test_louvain_paths_gpu import run
levels, res, out = int(sys.argv[1]), float(sys.argv[2]), sys.argv[3]
ops = gficf_amd.HipOps(0)
A = lf.nested_pairing_graph(levels)
N = A.shape[0]
p = dict(res=res, n_iter=1, algorithm=2, n_start=1, seed=0)
print("RUN canonical", file=sys.stderr, flush=True)
a = run(ops, N, *lf.canonical(A), **p)
print("RUN shuffled", file=sys.stderr, flush=True)
b = run(ops, N, *lf.form_shuffle(A, np.random.default_rng(13)), **p)
np.savez(out, la=a[0], lb=b[0], nq=np.asarray([a[1], b[1]]), q=np.asarray([a[2], b[2]]))
"""


@pytest.mark.parametrize("levels,res", [(15, 0.0), (16, 1e-7)])
def test_descent_deeper_than_the_saved_levels(levels, res, tmp_path):
    """tests/helpers/louvain_forms.nested_pairing_graph: every level of the descent merges the sibling blocks and nothing else, so the
    descent is as deep as the nesting.  The depth is read from the GFICF_LOUVAIN_DEBUG trace of a child process: level 13 and beyond
    have no saved map, the refinement begins at level 12 with what was found below it."""
    import re

    out = str(tmp_path / "deep.npz")
    env = dict(os.environ, PYTHONPATH=ROOT, GFICF_LOUVAIN_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", DEEP_CHILD, str(levels), repr(res), out], env=env, capture_output=True, text=True, timeout=280, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    for part in r.stderr.split("RUN ")[1:]:
        deepest = max(int(m) for m in re.findall(r"pass 0 level (\d+):", part))
        refined = sorted({int(m) for m in re.findall(r"pass 0 refinement level (\d+):", part)})
        print(part.split("\n")[0], "deepest level", deepest, "refinement levels", refined)
        assert deepest >= 13 and refined == list(range(13))
    z = np.load(out)
    A = lf.nested_pairing_graph(levels)
    a, b = (z["la"], int(z["nq"][0]), float(z["q"][0])), (z["lb"], int(z["nq"][1]), float(z["q"][1]))
    check_labels(A, as_cluster_labels(a), res)
    assert_same(b, a, ("nested pairing", levels, res))
    if res == 0.0:
        assert a[1] == 1 and a[2] == 1.0
    else:
        assert 1 < a[1] <= 1 << (levels - 13)                                # whole blocks of the levels below
        assert same_partition(a[0], np.arange(A.shape[0]) >> int(np.log2(A.shape[0] // a[1])))
