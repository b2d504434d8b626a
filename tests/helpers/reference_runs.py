"""The reference's modularity optimiser on the graphs the tests build, live or stored.

oracle.modularity_reference() runs oracle/_ref/modularity_optimizer, which build() compiles from the reference's own
src/ModularityOptimizer.cpp only where that source tree can be read.  So that the comparisons hold everywhere,
tests/golden/louvain_reference_runs.npz keeps, per case, what that binary returned (labels, the modularity it printed),
the arguments it was run with and a SHA-256 of the adjacency matrix it ran on (made by
tests/golden/make_louvain_reference_runs.py).  Where the binary is there it is run and must give the stored answer; where it
is not, the stored answer stands in for it, after the test's matrix is checked to be the one it was made on."""
import hashlib
import os

import numpy as np
import scipy.sparse as sp

import oracle

PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "louvain_reference_runs.npz")
_stored = None


def matrix_digest(A) -> str:
    A = sp.csc_matrix(A, copy=True)
    A.sort_indices()
    h = hashlib.sha256()
    for a in (np.asarray(A.shape, dtype=np.int64), A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.astype(np.float64)):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def params(resolution, algorithm, n_start, n_iter, seed, function):
    return np.array([resolution, algorithm, n_start, n_iter, seed, function], dtype=np.float64)


def stored():
    global _stored
    if _stored is None:
        z = np.load(PATH)
        _stored = {n: {f: z[n + "/" + f] for f in ("labels", "printed_q", "params", "digest")} for n in sorted({k.split("/")[0] for k in z.files})}
    return _stored


def modularity_reference(key, A, resolution, algorithm, n_start, n_iter, seed, function=1):
    """(labels, printed modularity) of the reference's optimiser on ``A`` with these arguments, as oracle.modularity_reference
    returns them: run live when the binary is built (and then held to the stored run of ``key``), the stored run otherwise."""
    run = stored().get(key)
    assert run is not None, f"no stored reference run '{key}' in {PATH}"
    assert np.array_equal(run["params"], params(resolution, algorithm, n_start, n_iter, seed, function)), (key, run["params"])
    assert str(run["digest"]) == matrix_digest(A), f"{key}: not the matrix the stored reference run was made on"
    if oracle.build_ref() is not None:
        labels, q = oracle.modularity_reference(A, resolution, algorithm, n_start, n_iter, seed, function=function)
        assert np.array_equal(labels, run["labels"]) and q == float(run["printed_q"]), key
        return labels, q
    return run["labels"].copy(), float(run["printed_q"])
