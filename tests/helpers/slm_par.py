"""The PARALLEL FORM of include/gficf_slm.h restated exactly: what libgficf_slm.so is meant to compute, bit for bit.

SLM is Leiden's level loop with another middle step, and so is this file: `Graph`, `Problem`, `local_moving`, `aggregate`,
`canonical` and `finish` are tests/helpers/leiden_par.py's, unchanged (plain Python integers, fragile decisions counted as there).
The sub-moving is `local_moving` from singletons on a Graph whose rows keep only the entries inside the vertex's own community (the
FENCE: no candidate, no weight and no stamp across it), with the vertex weights k of the full graph and the class hash of
seed ^ 0x27D4EB2F.  It shares no code with gficf_amd/csrc/slm.hip."""
import numpy as np

from tests.helpers.leiden_par import M32, MAX_LEVELS, Graph, Problem, accum, aggregate, canonical, finish, local_moving

SUB_SEED = 0x27D4EB2F


def fenced(g, comm):
    """g with the entries across the fence taken out; k untouched."""
    return Graph([{u: w for u, w in g.rows[v].items() if comm[u] == comm[v]} for v in range(g.n)], g.k)


def sub_moving(P, g, comm, level, seed):
    """(canonical sub-labels, passes): local moving from singletons inside the communities of comm."""
    sub, K, size = list(range(g.n)), g.k[:], [1] * g.n
    passes, _ = local_moving(P, fenced(g, comm), sub, K, size, level, (seed ^ SUB_SEED) & M32)
    return canonical(sub), passes


def iteration(P, start, seed, trace):
    g, comm, top = P.g0, canonical(start), list(range(P.N))
    for level in range(MAX_LEVELS):
        K, size = accum(g, comm)
        passes, qn = local_moving(P, g, comm, K, size, level, seed)
        n_comm = sum(1 for s in size if s > 0)
        rec = dict(level=level, vertices=g.n, passes=passes, communities=n_comm, q=P.q_float(qn), sub_passes=-1, sub=-1)
        trace.append(rec)
        if n_comm == g.n:
            break
        sub, rec["sub_passes"] = sub_moving(P, g, comm, level, seed)
        rec["sub"] = len(set(sub))
        if rec["sub"] == g.n:
            break
        g, comm, to = aggregate(g, comm, sub)
        top = [to[v] for v in top]
    return [comm[t] for t in top]


class Result:
    """labels int32 (clusters by decreasing size, ties by smallest member), n_clusters, modularity (the exact Q, rounded once), start,
    iterations (of that start), trace (of that start: one record a level), levels (records of its last iteration), fragile (over all
    starts) and exact_tie_cap."""


def one_start(P, seed, n_iter, init, early_stop=True):
    """(canonical labels, iterations run, trace, records of the last iteration)."""
    trace, lab, iterations, levels = [], canonical(list(range(P.N)) if init is None else [int(c) for c in init]), 0, 0
    for _ in range(n_iter):
        iterations += 1
        before = len(trace)
        new = canonical(iteration(P, lab, seed, trace))
        levels = len(trace) - before
        same, lab = new == lab, new
        if same and early_stop:             # it returned its own start: every further iteration would
            break
    return lab, iterations, trace, levels


def slm(A, resolution=0.8, n_start=10, n_iter=10, seed=0, init=None, early_stop=True):
    """early_stop=False runs all n_iter iterations (for showing that the early stop changes nothing)."""
    P = Problem(A, resolution)
    out = Result()
    out.start, out.iterations, out.trace, out.levels = 0, 0, [], 0
    if P.W2 == 0:
        lab = list(range(P.N))
    else:
        best = None
        for s in range(n_start):
            lab_s, iters, trace, levels = one_start(P, (seed + s) & M32, n_iter, init, early_stop)
            q = finish(P, lab_s)[2]
            if best is None or q > best[0]:
                best = (q, lab_s)
                out.start, out.iterations, out.trace, out.levels = s, iters, trace, levels
        lab = best[1]
    out.labels, out.n_clusters, out.modularity = finish(P, lab)
    out.fragile, out.exact_tie_cap = P.fragile, P.exact_tie_cap
    return out


def submove(A, labels, resolution=1.0, seed=0, level=0):
    """Step 3 alone on the finest graph under `labels` as they are: (int32 sub-labels = the smallest member, their number, passes,
    fragile count) — what gficf_slm_submove_* return."""
    P = Problem(A, resolution)
    if P.W2 == 0:
        return np.arange(P.N, dtype=np.int32), P.N, 0, 0
    sub, passes = sub_moving(P, P.g0, [int(c) for c in labels], level, seed & M32)
    return np.asarray(sub, dtype=np.int32), len(set(sub)), passes, P.fragile
