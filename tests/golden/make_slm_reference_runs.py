"""Generates tests/golden/slm_reference_runs.npz: what the REFERENCE's modularity optimiser returns with algorithm 3 (smart local
moving) on the graphs of tests/helpers/slm_cases.REFERENCE_CASES (read back by tests/helpers/slm_reference_runs.py).

Needs the binary build() makes in oracle/_ref/ from the reference's src/ModularityOptimizer.cpp (see oracle/Makefile); no GPU: the
graphs are built on the CPU.  Stored per case: the labels, the modularity the binary printed, its arguments (resolution,
algorithm 3, one start, ten iterations, seed 0, function 1) and the SHA-256 of the adjacency matrix.
Run from the repo root:  python tests/golden/make_slm_reference_runs.py [--out PATH]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import oracle  # noqa: E402
from oracle import oracle_np  # noqa: E402
from tests.helpers import reference_runs, slm_cases, slm_reference_runs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=slm_reference_runs.PATH)
    out_path = ap.parse_args().out
    if oracle.build_ref() is None:
        raise SystemExit("oracle/_ref/modularity_optimizer is not built: run build() where the reference's sources are readable")
    a = slm_reference_runs.ARGS
    out = {}
    for key in slm_cases.REFERENCE_CASES:
        A, res = slm_cases.reference_input(key)
        labels, q = oracle.modularity_reference(A, res, a["algorithm"], a["n_start"], a["n_iter"], a["seed"], function=a["function"])
        qn = oracle_np.modularity_np(A, labels, res, a["function"])
        assert abs(q - qn) < 6e-5, (key, q, qn)                  # the restated quality function against the reference's print-out
        print(f"{key}: N={A.shape[0]} nnz={A.nnz} clusters={labels.max() + 1} Q={qn:.6f} (printed {q})", flush=True)
        out[key + "/labels"] = labels.astype(np.int32)
        out[key + "/printed_q"] = np.float64(q)
        out[key + "/params"] = reference_runs.params(res, a["algorithm"], a["n_start"], a["n_iter"], a["seed"], a["function"])
        out[key + "/digest"] = np.str_(reference_runs.matrix_digest(A))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **out)


if __name__ == "__main__":
    main()
