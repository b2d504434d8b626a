"""The reference's modularity optimiser with algorithm 3 (SLM) on the graphs of tests/helpers/slm_cases.REFERENCE_CASES, live or
stored: tests/helpers/reference_runs.py's arrangement for tests/golden/slm_reference_runs.npz (made by
tests/golden/make_slm_reference_runs.py; the graphs need no device).  Where oracle/_ref/modularity_optimizer is built it is run
and held to the stored run; elsewhere the stored run stands in, after the test's matrix is checked to be the one it was made on."""
import os

import numpy as np

import oracle
from tests.helpers import reference_runs

PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "slm_reference_runs.npz")
ARGS = dict(algorithm=3, n_start=1, n_iter=10, seed=0, function=1)      # what every stored case was run with
_stored, _runs = None, {}


def stored():
    global _stored
    if _stored is None:
        z = np.load(PATH)
        _stored = {n: {f: z[n + "/" + f] for f in ("labels", "printed_q", "params", "digest")} for n in sorted({k.split("/")[0] for k in z.files})}
    return _stored


def slm_reference(key, A, resolution):
    """(labels, printed modularity) of the reference's algorithm 3 on ``A``: made once per process."""
    if key not in _runs:
        run = stored().get(key)
        assert run is not None, f"no stored reference run '{key}' in {PATH}"
        want = reference_runs.params(resolution, ARGS["algorithm"], ARGS["n_start"], ARGS["n_iter"], ARGS["seed"], ARGS["function"])
        assert np.array_equal(run["params"], want), (key, run["params"])
        assert str(run["digest"]) == reference_runs.matrix_digest(A), f"{key}: not the matrix the stored reference run was made on"
        if oracle.build_ref() is not None:
            labels, q = oracle.modularity_reference(A, resolution, ARGS["algorithm"], ARGS["n_start"], ARGS["n_iter"], ARGS["seed"], function=ARGS["function"])
            assert np.array_equal(labels, run["labels"]) and q == float(run["printed_q"]), key
        _runs[key] = (run["labels"].copy(), float(run["printed_q"]))
    return _runs[key]
