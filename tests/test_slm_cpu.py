"""No GPU: the header of libgficf_slm.so against its loader, the Makefile, the restatement (tests/helpers/slm_par.py) against the
reference optimiser's stored algorithm-3 runs (tests/golden/slm_reference_runs.npz), and the argument handling of the Python
mirror (everything it decides before the first call into the library)."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import gficf_amd
from gficf_amd import _slm_lib
from gficf_amd.api import COMMUNITY_ALGOS
from oracle import oracle_np
from tests.helpers import leiden_cases, slm_cases, slm_par, slm_reference_runs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_loader_name_the_same_entries():
    text = open(os.path.join(ROOT, "include", "gficf_slm.h")).read()
    body = text[text.index("extern \"C\""):]
    declared = re.findall(r"\b(gficf_slm_\w+)\s*\(([^;{}]*)\)\s*;", body)
    assert set(n for n, _ in declared) == set(_slm_lib.SIGNATURES) and len(declared) == 6
    for name, args in declared:
        n = 0 if args.strip() == "void" else args.count(",") + 1
        assert n == len(_slm_lib.SIGNATURES[name][1]), name
    assert "#define GFICF_SLM_ABI_VERSION 1" in text and _slm_lib.ABI_VERSION == 1
    # the structs, field for field
    for struct, cls in (("gficf_slm_info", _slm_lib.Info), ("gficf_slm_submove_info", _slm_lib.SubmoveInfo)):
        fields = re.findall(r"\b(?:int64_t|int32_t|double)\s+(\w+);", text[text.index("typedef struct " + struct):text.index("} " + struct)])
        assert fields == [f for f, _ in cls._fields_], struct
    # the libraries it stands beside keep their versions
    assert re.search(r"#define\s+GFICF_HIP_ABI_VERSION\s+7\b", open(os.path.join(ROOT, "include", "gficf_hip.h")).read())
    assert "#define GFICF_LEIDEN_ABI_VERSION 1" in open(os.path.join(ROOT, "include", "gficf_leiden.h")).read()


def test_makefile_builds_the_library_with_the_others():
    csrc = os.path.join(ROOT, "gficf_amd", "csrc")
    build = subprocess.run(["make", "-n", "-B", "-C", csrc, "all"], capture_output=True, text=True, check=True).stdout.splitlines()
    link = [ln for ln in build if " -o ../libgficf_slm.so " in ln]
    assert len(link) == 1 and re.search(r"hipcc --offload-arch=gfx950 -shared -fPIC -o \.\./libgficf_slm\.so slm\.o -L\.\. -lgficf_hip\b", link[0])
    comp = {n: [ln for ln in build if ln.endswith(f" -c {n}.hip -o {n}.o")] for n in ("slm", "leiden")}
    assert len(comp["slm"]) == 1 and comp["slm"][0].replace("slm", "leiden") == comp["leiden"][0]          # the flags of leiden.hip
    for n in ("slm", "leiden"):                                   # both are rebuilt when the header they share changes
        deps = subprocess.run(["make", "-n", "-W", "leiden_kernels.h", "-C", csrc, n + ".o"], capture_output=True, text=True, check=True).stdout
        assert f"-c {n}.hip" in deps
    clean = subprocess.run(["make", "-n", "-C", csrc, "clean"], capture_output=True, text=True, check=True).stdout
    assert re.search(r"^rm -f .*\bslm\.o\b.* \.\./libgficf_slm\.so\b", clean, re.M)


@pytest.mark.parametrize("key", slm_cases.REFERENCE_CASES)
def test_restatement_is_pinned_to_the_reference(key):
    """The reference's own algorithm 3 (seed 0, one start, ten iterations): the restatement reaches its Q within Q_TOL from below."""
    A, res = slm_cases.reference_input(key)
    ref, printed = slm_reference_runs.slm_reference(key, A, res)
    q_ref = oracle_np.modularity_np(A, ref, res)
    assert abs(printed - q_ref) < 6e-5, (key, printed, q_ref)
    run = slm_par.slm(A, res, 1, 10, 0)
    q = oracle_np.modularity_np(A, run.labels, res)
    print(key, "Q", q, "reference", q_ref, "iterations", run.iterations, "clusters", run.n_clusters, int(ref.max()) + 1)
    assert abs(q - run.modularity) < 1e-9
    assert q >= q_ref - slm_cases.Q_TOL, (key, q, q_ref)


def test_stored_runs_are_algorithm_3():
    runs = slm_reference_runs.stored()
    assert sorted(runs) == sorted(slm_cases.REFERENCE_CASES)
    for key, run in runs.items():
        assert run["params"][1:].tolist() == [3, 1, 10, 0, 1], key


def test_mirror_rejects_bad_arguments():
    A, _ = leiden_cases.ring(8, 5)
    bad = [dict(n_start=0), dict(n_iter=0), dict(resolution=-0.5), dict(resolution=float("nan")), dict(resolution=float("inf")),
           dict(init=np.zeros(7, dtype=np.int32)), dict(init=np.full(40, 40, dtype=np.int32)), dict(init=np.full(40, -1, dtype=np.int32))]
    for kw in bad:
        with pytest.raises(ValueError):
            gficf_amd.slm(A, **kw)
    with pytest.raises(ValueError):
        gficf_amd.slm(sp.csc_matrix((4, 5)))
    P = np.zeros(40, dtype=np.int32)
    for args, kw in (((A, P[:3]), {}), ((A, np.full(40, 40)), {}), ((A, P), dict(level=-1)), ((A, P), dict(resolution=-1.0)),
                     ((sp.csc_matrix((4, 5)), P[:4]), {})):
        with pytest.raises(ValueError):
            gficf_amd.slm_submove(*args, **kw)


def test_community_algos_and_the_refusals_that_stay():
    assert "slm" in COMMUNITY_ALGOS and "walktrap" not in COMMUNITY_ALGOS and "fastgreedy" not in COMMUNITY_ALGOS
    for algo in ("nope", "walktrap", "fastgreedy"):
        with pytest.raises(ValueError, match="walktrap.*fastgreedy"):
            gficf_amd.clustcells({"pca": {"cells": np.zeros((4, 2))}}, community_algo=algo)
    with pytest.raises(ValueError, match=r"slm\(\)"):
        gficf_amd.run_modularity_clustering(leiden_cases.ring(8, 5)[0], 1, 0.8, 3)
