"""No GPU: the header of libgficf_leiden.so against its loader, the Makefile, the NumPy restatement of the algorithm
(tests/helpers/leiden_np.py, the yardstick of tests/test_leiden_gpu.py) against the reference optimiser's stored results, and
the argument handling of the Python mirror (everything it decides before the first call into the library)."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import gficf_amd
from gficf_amd import _leiden_lib
from gficf_amd.api import COMMUNITY_ALGOS
from oracle import oracle_np
from tests.helpers import closed_form, leiden_cases, leiden_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_loader_name_the_same_entries():
    text = open(os.path.join(ROOT, "include", "gficf_leiden.h")).read()
    body = text[text.index("extern \"C\""):]
    declared = re.findall(r"\b(gficf_leiden_\w+)\s*\(([^;]*)\)\s*;", body)
    assert set(n for n, _ in declared) == set(_leiden_lib.SIGNATURES) and len(declared) == 7
    for name, args in declared:
        n = 0 if args.strip() == "void" else args.count(",") + 1
        assert n == len(_leiden_lib.SIGNATURES[name][1]), name
    assert "#define GFICF_LEIDEN_ABI_VERSION 1" in text and _leiden_lib.ABI_VERSION == 1
    core = open(os.path.join(ROOT, "include", "gficf_hip.h")).read()
    assert re.search(r"#define\s+GFICF_HIP_ABI_VERSION\s+7\b", core)


def test_makefile_builds_the_library_with_the_others():
    # what make itself would run (a dry run of everything, nothing is compiled): the rules are free to be shared with the other add-ons
    csrc = os.path.join(ROOT, "gficf_amd", "csrc")
    build = subprocess.run(["make", "-n", "-B", "-C", csrc, "all"], capture_output=True, text=True, check=True).stdout.splitlines()
    link = [ln for ln in build if " -o ../libgficf_leiden.so " in ln]
    assert len(link) == 1 and re.search(r"hipcc --offload-arch=gfx950 -shared -fPIC -o \.\./libgficf_leiden\.so leiden\.o -L\.\. -lgficf_hip\b", link[0])
    assert build.index(link[0]) > max(i for i, ln in enumerate(build) if " -o ../libgficf_hip.so " in ln or ln.endswith(" -o leiden.o"))
    clean = subprocess.run(["make", "-n", "-C", csrc, "clean"], capture_output=True, text=True, check=True).stdout
    assert re.search(r"^rm -f .*\bleiden\.o\b.* \.\./libgficf_leiden\.so\b", clean, re.M)


@pytest.mark.parametrize("name", ["knn_blobs", "knn_noise_alg2", "planted3", "planted8_res08"])
def test_restatement_on_the_golden_graphs(name):
    A, res, ref = leiden_cases.golden()[name]
    q_ref = oracle_np.modularity_np(A, ref, res)
    for n_iterations in (1, 2):
        lab = leiden_np.leiden(A, res, n_iterations)
        assert abs(leiden_np.modularity(A, lab, res) - oracle_np.modularity_np(A, lab, res)) < 1e-12
        assert leiden_np.communities_connected(A, lab)
        if name != "knn_noise_alg2":
            assert leiden_np.same_partition(lab, ref), (name, n_iterations)
    if name == "knn_noise_alg2":
        assert abs(leiden_np.modularity(A, lab, res) - 0.6575) < 5e-5 and abs(q_ref - 0.6548) < 5e-5
    if name != "planted3":
        P = leiden_np.local_moving(A, np.arange(A.shape[0]), res)
        R = leiden_np.refine(A, P, res)
        assert leiden_np.refine_leftover(A, P, R, res, 1e-6) == 0 and len(np.unique(R)) < A.shape[0]
        assert leiden_np.refine_leftover(A, P, np.arange(A.shape[0]), res, 1e-6) > 0      # the guard sees the trivial answer


@pytest.mark.parametrize("c,m", leiden_cases.RINGS)
def test_restatement_on_the_rings(c, m):
    A, clique = leiden_cases.ring(c, m)
    lab = leiden_np.leiden(A, 0.8, 2)
    assert len(np.unique(lab)) == c and leiden_np.same_partition(lab, clique)
    assert abs(leiden_np.modularity(A, lab, 0.8) - closed_form.ring_of_cliques_modularity(c, m, 0.8)) < 1e-12
    assert round(closed_form.ring_of_cliques_modularity(c, m, 0.8), 4) == {8: 0.8091, 60: 0.9649}[c]
    # a community of two components: local moving alone keeps it, the refinement splits it
    _, _, init = leiden_cases.disconnected_start(c, m)
    assert not leiden_np.communities_connected(A, init)
    assert leiden_np.same_partition(leiden_np.local_moving(A, init, 0.8), init)
    assert leiden_np.same_partition(leiden_np.refine(A, init, 0.8), clique)


def test_mirror_rejects_bad_arguments():
    A, _ = leiden_cases.ring(8, 5)
    with pytest.raises(ValueError):
        gficf_amd.leiden(A, 0.8, n_iterations=0)
    with pytest.raises(ValueError):
        gficf_amd.leiden(A, -0.5)
    with pytest.raises(ValueError):
        gficf_amd.leiden(A, float("nan"))
    with pytest.raises(ValueError):
        gficf_amd.leiden(A, 0.8, init=np.zeros(7, dtype=np.int32))
    with pytest.raises(ValueError):
        gficf_amd.leiden(A, 0.8, init=np.full(40, 40, dtype=np.int32))
    with pytest.raises(ValueError):
        gficf_amd.leiden(sp.csc_matrix((4, 5)), 0.8)
    with pytest.raises(ValueError):
        gficf_amd.leiden_refine(A, np.zeros(3, dtype=np.int32), 0.8)
    with pytest.raises(ValueError):
        gficf_amd.leiden_refine(sp.csc_matrix((4, 5)), np.zeros(4, dtype=np.int32))


def test_community_algos():
    assert "leiden" in COMMUNITY_ALGOS and "walktrap" not in COMMUNITY_ALGOS and "fastgreedy" not in COMMUNITY_ALGOS
    for algo in ("walktrap", "fastgreedy"):
        with pytest.raises(ValueError, match="walktrap.*fastgreedy"):
            gficf_amd.clustcells({"pca": {"cells": np.zeros((4, 2))}}, community_algo=algo)
