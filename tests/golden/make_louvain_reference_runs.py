"""Generates tests/golden/louvain_reference_runs.npz: what the REFERENCE's modularity optimiser returns on the graphs that
tests/test_louvain_gpu.py and tests/test_oracle.py hand it (read back by tests/helpers/reference_runs.py).

Needs the binary build() makes in oracle/_ref/ from the reference's src/ModularityOptimizer.cpp (see oracle/Makefile), and a
GPU: the kNN -> Jaccard graphs are built by the device chain, exactly as the tests build them.  Stored per case: the labels, the
modularity the binary printed, its arguments (resolution, algorithm, n_start, n_iter, seed, function) and the SHA-256 of the
adjacency matrix.  Run from the repo root:  python tests/golden/make_louvain_reference_runs.py [--out PATH]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import oracle  # noqa: E402
from oracle import oracle_np  # noqa: E402
from tests.helpers import closed_form, reference_runs  # noqa: E402


def cases():
    """(key, graph builder, resolution, algorithm, n_start, n_iter, seed, function): the calls the tests make."""
    from tests import test_louvain_gpu as t

    out = []
    for N, d, k, C, res in t.LIVE_CASES:
        out.append((f"live_N{N}_d{d}_k{k}_C{C}_res{res}", lambda N=N, d=d, k=k, C=C: t.knn_graph(N, d, k, C, seed=N + k), res, 1, 1, 10, 0, 1))
    out.append(("large_200k", lambda: t.knn_graph(200000, 20, 30, 40, seed=77, spread=2.0), 0.8, 1, 1, 10, 0, 1))
    for N, k, C, res in t.FUNCTION2_CASES:
        out.append((f"function2_N{N}_k{k}_C{C}_res{res}", lambda N=N, k=k, C=C: t.knn_graph(N, 10, k, C, seed=N + k), res, 1, 1, 10, 0, 2))
    out.append(("hubs", t.hub_graph, 1.0, 1, 1, 10, 0, 1))
    out.append(("resolution_alg2", lambda: t.knn_graph(5000, 10, 15, 1, seed=11), 1.0, 2, 1, 10, 0, 1))
    for c, m in ((8, 5), (60, 10), (200, 20)):                       # tests/test_oracle.py, the ring of cliques
        out.append((f"ring_c{c}_m{m}", lambda c=c, m=m: closed_form.ring_of_cliques(c, m, 0.37)[0], 0.8, 1, 10, 10, 0, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=reference_runs.PATH)
    out_path = ap.parse_args().out
    if oracle.build_ref() is None:
        raise SystemExit("oracle/_ref/modularity_optimizer is not built: run build() where the reference's sources are readable")
    out = {}
    for key, graph, res, alg, n_start, n_iter, seed, function in cases():
        A = graph()
        labels, q = oracle.modularity_reference(A, res, alg, n_start, n_iter, seed, function=function)
        qn = oracle_np.modularity_np(A, labels, res, function)
        assert abs(q - qn) < 6e-5, (key, q, qn)                  # the restated quality function against the reference's print-out
        print(f"{key}: N={A.shape[0]} nnz={A.nnz} clusters={labels.max() + 1} Q={qn:.6f} (printed {q})", flush=True)
        out[key + "/labels"] = labels.astype(np.int32)
        out[key + "/printed_q"] = np.float64(q)
        out[key + "/params"] = reference_runs.params(res, alg, n_start, n_iter, seed, function)
        out[key + "/digest"] = np.str_(reference_runs.matrix_digest(A))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **out)


if __name__ == "__main__":
    main()
