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
