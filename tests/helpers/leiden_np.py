"""A sequential NumPy / SciPy restatement of the Leiden algorithm as include/gficf_leiden.h states it, written from the paper's
description (Traag, Waltman, van Eck 2019): vertices in id order, a queue for the local moving, one refinement pass in id order
with the largest gain and ties to the smaller label, aggregation by the refined partition.  The yardstick of
tests/test_leiden_gpu.py and the subject of tests/test_leiden_cpu.py; it shares no code with the device path."""
from collections import deque

import numpy as np
import scipy.sparse as sp
from scipy.sparse import csgraph


def _graph(A):
    A = sp.csr_matrix(A).astype(np.float64).copy()
    A.setdiag(0.0)
    A.eliminate_zeros()
    return A


def modularity(A, labels, resolution=1.0):
    """Q = (1/2W) [ sum_ij A_ij delta(c_i, c_j) - resolution * sum_c K_c^2 / 2W ], the diagonal ignored."""
    A = _graph(A)
    lab = np.asarray(labels)
    k = np.asarray(A.sum(axis=1)).ravel()
    two_w = k.sum()
    if two_w == 0:
        return 0.0
    coo = A.tocoo()
    inside = coo.data[lab[coo.row] == lab[coo.col]].sum()
    K = np.bincount(lab, weights=k)
    return float((inside - resolution * (K * K).sum() / two_w) / two_w)


def canonical(labels):
    """Every community labelled by its smallest member."""
    lab = np.asarray(labels, dtype=np.int64)
    first = np.full(lab.max() + 1 if len(lab) else 0, len(lab), dtype=np.int64)
    np.minimum.at(first, lab, np.arange(len(lab)))
    return first[lab]


def _row_weights(G, v, comm, only=None):
    """Weight from v to every label of `comm` among its neighbours (self-loops are not edges); `only`: a mask of neighbours."""
    out = {}
    for e in range(G.indptr[v], G.indptr[v + 1]):
        u = G.indices[e]
        if u == v or G.data[e] == 0 or (only is not None and not only[u]):
            continue
        out[comm[u]] = out.get(comm[u], 0.0) + G.data[e]
    return out


def _local_move(G, k, comm, r):
    n = G.shape[0]
    comm = comm.copy()
    K = np.bincount(comm, weights=k, minlength=n)
    queue, queued = deque(range(n)), np.ones(n, dtype=bool)
    while queue:
        v = queue.popleft()
        queued[v] = False
        w = _row_weights(G, v, comm)
        cv = comm[v]
        K[cv] -= k[v]
        best, best_gain = cv, w.get(cv, 0.0) - r * k[v] * K[cv]
        for c in sorted(w):
            gain = w[c] - r * k[v] * K[c]
            if gain > best_gain or (gain == best_gain and c < best):
                best, best_gain = c, gain
        K[best] += k[v]
        if best != cv:
            comm[v] = best
            for e in range(G.indptr[v], G.indptr[v + 1]):
                u = G.indices[e]
                if u != v and comm[u] != best and not queued[u]:
                    queue.append(u)
                    queued[u] = True
    return comm


def _refine(G, k, comm, r):
    n = G.shape[0]
    K = np.bincount(comm, weights=k, minlength=n)
    ref = np.arange(n)
    rsize, Kr = np.ones(n, dtype=np.int64), k.astype(np.float64).copy()
    ec = np.zeros(n)
    for v in range(n):
        ec[v] = _row_weights(G, v, comm).get(comm[v], 0.0)
    ext = ec.copy()
    for v in range(n):
        KC = K[comm[v]]
        if rsize[ref[v]] != 1 or ec[v] < r * k[v] * (KC - k[v]):
            continue
        w = _row_weights(G, v, ref, only=(comm == comm[v]))
        best, best_gain = -1, 0.0
        for t in sorted(w):
            if t == ref[v] or ext[t] < r * Kr[t] * (KC - Kr[t]):
                continue
            gain = w[t] - r * k[v] * Kr[t]
            if gain >= 0 and (best < 0 or gain > best_gain):
                best, best_gain = t, gain
        if best >= 0:
            ext[best] += ec[v] - 2.0 * w[best]
            Kr[best] += k[v]
            rsize[best] += 1
            old = ref[v]
            ref[v] = best
            rsize[old], Kr[old], ext[old] = 0, 0.0, 0.0
    return ref


def local_moving(A, labels, resolution=1.0):
    """The local-moving stage alone from `labels` on the finest graph."""
    G = _graph(A)
    k = np.asarray(G.sum(axis=1)).ravel()
    return _local_move(G, k, canonical(labels), resolution / k.sum())


def refine(A, labels, resolution=1.0):
    """The refinement stage alone; every refined community labelled by its smallest member."""
    G = _graph(A)
    k = np.asarray(G.sum(axis=1)).ravel()
    return canonical(_refine(G, k, np.asarray(labels, dtype=np.int64), resolution / k.sum()))


def _iteration(G, k, labels, r):
    N = G.shape[0]
    n, top, comm = N, np.arange(N), canonical(labels)
    while True:
        comm = _local_move(G, k, comm, r)
        if len(np.unique(comm)) == n:
            break
        ref = _refine(G, k, comm, r)
        uniq, newid = np.unique(ref, return_inverse=True)
        n2 = len(uniq)
        if n2 == n:
            break
        S = sp.csr_matrix((np.ones(n), (np.arange(n), newid)), shape=(n, n2))
        G = sp.csr_matrix(S.T @ G @ S)
        k = np.asarray(S.T @ k).ravel()
        comm2 = np.zeros(n2, dtype=np.int64)
        comm2[newid] = comm
        comm, top, n = canonical(comm2), newid[top], n2
    return comm[top]


def leiden(A, resolution=1.0, n_iterations=2, init=None):
    """Labels (a community's label is its smallest member) after `n_iterations` iterations from `init` (None: singletons)."""
    G = _graph(A)
    N = G.shape[0]
    k = np.asarray(G.sum(axis=1)).ravel()
    if k.sum() == 0:
        return np.arange(N)
    labels = np.arange(N) if init is None else np.asarray(init, dtype=np.int64)
    for _ in range(n_iterations):
        labels = canonical(_iteration(G, k, labels, resolution / k.sum()))
    return labels


def same_partition(a, b):
    pairs = np.unique(np.stack([np.asarray(a), np.asarray(b)], axis=1), axis=0)
    return len(pairs) == len(np.unique(a)) == len(np.unique(b))


def communities_connected(A, labels):
    """Every community's induced subgraph (off-diagonal, positive entries) has one component."""
    C = sp.coo_matrix(_graph(A))
    lab = np.asarray(labels, dtype=np.int64)
    N = len(lab)
    keep = (lab[C.row] == lab[C.col]) & (C.data > 0)
    G = sp.csr_matrix((np.ones(int(keep.sum()), dtype=np.int8), (C.row[keep], C.col[keep])), shape=(N, N))
    n_comp, _ = csgraph.connected_components(G, directed=False)
    return n_comp == len(np.unique(lab))


def refine_leftover(A, P, R, resolution=1.0, tol=1e-6):
    """Vertices the refinement R of the partition P should still have moved: alone in their refined community, well connected to
    their community, and with an edge to a well-connected refined community of their community at a gain above `tol` (weight
    units).  0 for a finished refinement; what rules out the trivial answer "all singletons"."""
    G = _graph(A)
    P, R = np.asarray(P, dtype=np.int64), np.asarray(R, dtype=np.int64)
    N = G.shape[0]
    k = np.asarray(G.sum(axis=1)).ravel()
    r = resolution / k.sum()
    K = np.bincount(P, weights=k, minlength=N)
    Kr = np.bincount(R, weights=k, minlength=N)
    rsize = np.bincount(R, minlength=N)
    coo = G.tocoo()
    out = (P[coo.row] == P[coo.col]) & (R[coo.row] != R[coo.col])
    ext = np.bincount(R[coo.row[out]], weights=coo.data[out], minlength=N)           # E(r, C - r)
    same = P[coo.row] == P[coo.col]
    ec = np.bincount(coo.row[same], weights=coo.data[same], minlength=N)              # e(v, C - v)
    left = 0
    for v in np.flatnonzero(rsize[R] == 1):
        KC = K[P[v]]
        if ec[v] < r * k[v] * (KC - k[v]):
            continue
        w = _row_weights(G, v, R, only=(P == P[v]))
        for t, e in w.items():
            if t != R[v] and ext[t] >= r * Kr[t] * (KC - Kr[t]) and e - r * k[v] * Kr[t] > tol:
                left += 1
                break
    return left
