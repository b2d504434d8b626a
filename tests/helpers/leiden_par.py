"""The PARALLEL FORM of include/gficf_leiden.h restated exactly: what libgficf_leiden.so is meant to compute, bit for bit.

Plain Python on Python integers, written from the header's comment; it shares no code with gficf_amd/csrc/leiden.hip and runs on the
CPU.  Weights are rint(x * 2^32); the resolution is the exact fraction num / den of the double that is passed; a gain
e - (num / den) k K / 2W is compared after multiplying through by D = den * 2W, Q as inw * 2W * den - num * sum K^2 over den * (2W)^2.
No decision is taken in floating point, so wherever the device's f64 evaluation is not in doubt the two must agree on every label.

Where it IS in doubt the restatement counts a FRAGILE decision (the `fragile` field of a result): the exact tests of
tests/test_leiden_exact_gpu.py use only inputs whose count is 0 (tests/test_leiden_par_cpu.py asserts that for each of them).
  * a comparison of two gains, of a gain with the stay value, or one of the refinement's >= tests is fragile when its two sides are not
    built from identical operands (then the device computes identical doubles and ties as the integers do) and differ by at most
    2^-40 of the summed magnitudes of their terms: the device forms a side with at most four roundings of 2^-53 relative each and
    possibly one fused multiply-add, which 2^-40 covers with a factor of about 2^11 to spare;
  * the undo decision of a pass of local moving is fragile when something moved and |dQ| < 1e-9: the device adds at most n + 1024
    doubles into sum K^2 (relative error about n 2^-53, 1e-12 at n = 2^13), which 1e-9 covers a thousand times.

Entries of weight 0 (stored zeros, and the diagonal at level 0) are dropped when the graph is read: they are no edges, they carry no
stamp, and no sum sees them.  The row lengths, which select the device's kernels, do not appear here at all."""
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

SCALE = 4294967296.0
SUB, MAX_PASSES, MAX_LEVELS = 4, 64, 64
M32 = 0xFFFFFFFF
EPS_SHIFT = 40                  # a comparison within 2^-40 of its terms' magnitudes is fragile
DQ_FRAGILE = 10 ** 9            # |dQ| < 1e-9 with something moved is fragile


def hash32(v):
    v &= M32
    v ^= v >> 16; v = (v * 0x7feb352d) & M32
    v ^= v >> 15; v = (v * 0x846ca68b) & M32
    v ^= v >> 16
    return v


def level_seed(seed, level):
    return hash32((seed * 0x9E3779B1 + level * 0x85EBCA77 + 0x165667B1) & M32)


class Graph:
    """rows[v]: {u: weight} over the entries of non-zero weight (u == v: a self-loop of a coarser level), k[v]: the vertex weight,
    stamps[v]: whom a move of v stamps — the targets of rows[v], as the header rules."""

    def __init__(self, rows, k, stamps=None):
        self.n, self.rows, self.k, self.stamps = len(rows), rows, k, rows if stamps is None else stamps


class Problem:
    """stamp_stored: the rule the header excludes, for showing that it matters (tests/test_leiden_par_cpu.py) — at level 0 a mover
    stamps the target of EVERY stored entry, stored zeros and the diagonal included."""

    def __init__(self, A, resolution, stamp_stored=False):
        if isinstance(A, tuple):
            indptr, indices, x = A
        else:
            A = sp.csc_matrix(A)
            indptr, indices, x = A.indptr, A.indices, A.data
        N = len(indptr) - 1
        f = np.rint(np.asarray(x, dtype=np.float64) * SCALE).astype(np.int64).tolist()
        idx, ptr = np.asarray(indices).tolist(), np.asarray(indptr).tolist()
        rows = []
        for v in range(N):
            row = {}
            for e in range(ptr[v], ptr[v + 1]):
                if idx[e] != v and f[e]:
                    row[idx[e]] = row.get(idx[e], 0) + f[e]
            rows.append(row)
        stored = [set(idx[ptr[v]:ptr[v + 1]]) for v in range(N)] if stamp_stored else None
        self.g0 = Graph(rows, [sum(r.values()) for r in rows], stored)
        self.N, self.W2 = N, sum(self.g0.k)
        self.num, self.den = float(resolution).as_integer_ratio()
        self.D = self.den * self.W2
        self.fragile = 0
        self.exact_tie_cap = 0          # levels that ran all MAX_PASSES passes with dQ == 0 between the last two

    def close(self, diff, mag, identical):
        """Count and report a fragile comparison: sides `diff` apart whose terms have magnitudes adding up to `mag`."""
        if identical or mag == 0 or (abs(diff) << EPS_SHIFT) > mag:
            return False
        self.fragile += 1
        return True

    def q_num(self, g, comm, K):
        inw = 0
        for v, row in enumerate(g.rows):
            cv = comm[v]
            for u, w in row.items():
                if u == v or comm[u] == cv:
                    inw += w
        return inw * self.D - self.num * sum(k * k for k in K)

    def q_float(self, qn):
        return float(Fraction(qn, self.den * self.W2 * self.W2)) if self.W2 else 0.0


def canonical(lab):
    first = {}
    for v, c in enumerate(lab):
        if c not in first:
            first[c] = v
    return [first[c] for c in lab]


def accum(g, comm):
    K, size = [0] * g.n, [0] * g.n
    for v, c in enumerate(comm):
        K[c] += g.k[v]
        size[c] += 1
    return K, size


def local_moving(P, g, comm, K, size, level, seed):
    """In place on (comm, K, size).  Returns (passes, Q numerator of the result)."""
    hseed = level_seed(seed, level)
    cls = [hash32(v ^ hseed) % SUB for v in range(g.n)]
    mark = [0] * g.n
    D, num = P.D, P.num
    q_prev = P.q_num(g, comm, K)
    t = passes = 0
    for _ in range(MAX_PASSES):
        passes += 1
        snap = (comm[:], K[:], size[:])
        moved = False
        for s in range(SUB):
            t += 1
            moves = []
            for v in range(g.n):
                if cls[v] != s or not (t <= SUB or mark[v] >= t - SUB):
                    continue
                cv, kv = comm[v], g.k[v]
                e = {}
                for u, w in g.rows[v].items():
                    if u != v:
                        e[comm[u]] = e.get(comm[u], 0) + w
                stay_e = e.pop(cv, 0)
                if not e:
                    continue
                nk = num * kv
                cand = [(w * D - nk * K[c], -c, w, K[c]) for c, w in e.items()]
                bg, nbc, be, bK = max(cand)
                bc = -nbc
                for gc, _, w, Kc in cand:
                    P.close(bg - gc, (be + w) * D + nk * (bK + Kc), (w, Kc) == (be, bK))
                Ks = K[cv] - kv
                gs = stay_e * D - nk * Ks
                P.close(bg - gs, (be + stay_e) * D + nk * (bK + Ks), (be, bK) == (stay_e, Ks))
                mv = bg > gs or (bg == gs and bc < cv)
                if mv and size[cv] == 1 and size[bc] == 1 and bc > cv:
                    mv = False
                if mv:
                    moves.append((v, bc))
            for v, bc in moves:
                old, kv = comm[v], g.k[v]
                comm[v] = bc
                K[bc] += kv; K[old] -= kv
                size[bc] += 1; size[old] -= 1
                for u in g.stamps[v]:           # entries of non-zero weight only: a stored zero carries no stamp
                    mark[u] = t
            moved = moved or bool(moves)
        q = P.q_num(g, comm, K)
        if not moved:
            break
        if abs(q - q_prev) * DQ_FRAGILE < P.den * P.W2 * P.W2:
            P.fragile += 1
            if q == q_prev and passes == MAX_PASSES:
                P.exact_tie_cap += 1
        if q < q_prev:
            comm[:], K[:], size[:] = snap
            break
        q_prev = q
    return passes, q_prev


def refinement(P, g, comm, K):
    """(ref, rounds): ref[v] = the label of v's refined community, a member of it with ref[label] == label."""
    n, D, num = g.n, P.D, P.num
    ref, rsize, Kr = list(range(n)), [1] * n, g.k[:]
    inside = [{u: w for u, w in g.rows[v].items() if u != v and comm[u] == comm[v]} for v in range(n)]
    ec = [sum(r.values()) for r in inside]
    ext = ec[:]
    rounds = 0
    for _ in range(n + 1):
        rounds += 1
        prop = [-1] * n
        for v in range(n):
            if rsize[ref[v]] != 1:
                continue
            kv, Kc = g.k[v], K[comm[v]]
            lhs, rhs = ec[v] * D, num * kv * (Kc - kv)
            P.close(lhs - rhs, lhs + rhs, False)
            if lhs < rhs:
                continue
            e = {}
            for u, w in inside[v].items():
                e[ref[u]] = e.get(ref[u], 0) + w
            cand = []
            for c, w in e.items():
                if not (rsize[c] > 1 or c < v):
                    continue
                kr = Kr[c]
                lhs, rhs = ext[c] * D, num * kr * (Kc - kr)
                P.close(lhs - rhs, lhs + rhs, False)
                if lhs < rhs:
                    continue
                lhs, rhs = w * D, num * kv * kr
                P.close(lhs - rhs, lhs + rhs, False)
                if lhs >= rhs:
                    cand.append((lhs - rhs, -c, w, kr))
            if cand:
                bg, nbc, be, bk = max(cand)
                for gc, _, w, kr in cand:
                    P.close(bg - gc, (be + w) * D + num * kv * (bk + kr), (w, kr) == (be, bk))
                prop[v] = -nbc
        commits = [(v, p) for v, p in enumerate(prop) if p >= 0 and prop[p] < 0]
        if not commits:
            break
        for v, p in commits:
            ref[v] = p
            rsize[p] += 1; rsize[v] = 0
            Kr[p] += g.k[v]; Kr[v] = 0
        ext = [0] * n
        for v in range(n):
            rv = ref[v]
            ext[rv] += sum(w for u, w in inside[v].items() if ref[u] != rv)
    return ref, rounds


def aggregate(g, comm, ref):
    """The refined communities, in ascending order of their labels, as the vertices of the next level."""
    newid, n2 = {}, 0
    for v in range(g.n):
        if ref[v] == v:
            newid[v] = n2
            n2 += 1
    to = [newid[ref[v]] for v in range(g.n)]
    rows, k = [{} for _ in range(n2)], [0] * n2
    cmin = {}
    for v in range(g.n):
        R = to[v]
        k[R] += g.k[v]
        row = rows[R]
        for u, w in g.rows[v].items():
            row[to[u]] = row.get(to[u], 0) + w
        cmin[comm[v]] = min(cmin.get(comm[v], n2), R)
    comm2 = [0] * n2
    for v in range(g.n):
        comm2[to[v]] = cmin[comm[v]]
    return Graph(rows, k), comm2, to


def iteration(P, start, seed, trace):
    g, comm, top = P.g0, canonical(start), list(range(P.N))
    for level in range(MAX_LEVELS):
        K, size = accum(g, comm)
        passes, qn = local_moving(P, g, comm, K, size, level, seed)
        n_comm = sum(1 for s in size if s > 0)
        rec = dict(level=level, vertices=g.n, passes=passes, communities=n_comm, q=P.q_float(qn), rounds=None, refined=None)
        trace.append(rec)
        if n_comm == g.n:
            break
        ref, rounds = refinement(P, g, comm, K)
        n2 = sum(1 for v in range(g.n) if ref[v] == v)
        rec["rounds"], rec["refined"] = rounds, n2
        if n2 == g.n:
            break
        g, comm, to = aggregate(g, comm, ref)
        top = [to[v] for v in top]
    return [comm[t] for t in top]


class Result:
    """labels int32 (clusters by decreasing size, ties by smallest member), n_clusters, modularity (the exact Q, rounded once), the
    per-level trace, the fragile count, and how many levels ended at the pass cap on an exact tie of Q."""


def finish(P, lab):
    """(labels int32 numbered by decreasing size with ties by smallest member, n_clusters, exact Q) of canonical labels."""
    K, size = accum(P.g0, lab)
    order = sorted((c for c in range(P.N) if size[c] > 0), key=lambda c: (-size[c], c))
    rank = {c: i for i, c in enumerate(order)}
    return np.asarray([rank[c] for c in lab], dtype=np.int32), len(order), P.q_float(P.q_num(P.g0, lab, K)) if P.W2 else 0.0


def leiden(A, resolution=1.0, n_iterations=2, seed=0, init=None, stamp_stored=False):
    """The result of n_iterations iterations; .after[i]: (labels, n_clusters, modularity) had the run ended after iteration i + 1,
    .levels[i]: how many records of .trace the first i + 1 iterations wrote."""
    P = Problem(A, resolution, stamp_stored)
    out = Result()
    out.trace, out.after, out.levels = [], [], []
    if P.W2 == 0:
        lab = list(range(P.N))
    else:
        lab = list(range(P.N)) if init is None else [int(c) for c in init]
        for _ in range(n_iterations):
            lab = canonical(iteration(P, lab, seed & M32, out.trace))
            out.after.append(finish(P, lab))
            out.levels.append(len(out.trace))
    out.labels, out.n_clusters, out.modularity = out.after[-1] if out.after else finish(P, lab)
    out.fragile, out.exact_tie_cap = P.fragile, P.exact_tie_cap
    return out


def refine(A, labels, resolution=1.0):
    """The refinement alone on the caller's partition (labels in [0, N), as they are): (int32 labels = the smallest member of every
    refined community, their number, rounds, fragile count) — what gficf_leiden_refine_* return."""
    P = Problem(A, resolution)
    comm = [int(c) for c in labels]
    if P.W2 == 0:
        return np.arange(P.N, dtype=np.int32), P.N, 0, 0
    K, _ = accum(P.g0, comm)
    ref, rounds = refinement(P, P.g0, comm, K)
    return np.asarray(canonical(ref), dtype=np.int32), len(set(ref)), rounds, P.fragile


def move(A, labels, resolution=1.0, seed=0, level=0):
    """Local moving alone on the finest graph from `labels` (made canonical): (labels, passes, exact Q, fragile count)."""
    P = Problem(A, resolution)
    comm = canonical([int(c) for c in labels])
    K, size = accum(P.g0, comm)
    passes, qn = local_moving(P, P.g0, comm, K, size, level, seed & M32)
    return np.asarray(comm, dtype=np.int32), passes, P.q_float(qn), P.fragile
