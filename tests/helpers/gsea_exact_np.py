"""Yardsticks of libgficf_gsea_exact.so (include/gficf_gsea_exact.h): the one-sided tail of the enrichment score at gseaParam = 0.

``tail_exact`` counts with Python integers, walking forward as the contract defines the tail; ``tail_enumerated`` lists every
subset; ``tail_f64`` is the f64 port of the library's recurrence, lane by lane and in its order of additions (both sides run
the first-passage walk, the negative side through the mirrored set), so its bits are the library's."""
from fractions import Fraction
from itertools import combinations
from math import comb

import numpy as np

LANES = 64
MAX_SIZE = 4095


def top(i, j, G, m):
    """fl(fl(i / m) - fl(j / (G - m))): i the 1-based hit index, j the misses before it (arrays or scalars)."""
    return np.asarray(i, dtype=np.float64) / np.float64(m) - np.asarray(j, dtype=np.float64) / np.float64(G - m)


def bottom(i, j, G, m):
    return top(i, j, G, m) - np.float64(1.0) / np.float64(m)


def max_min(S, G):
    """(maxP, minP) of the set with ascending 1-based positions S among G."""
    S = np.asarray(S, dtype=np.int64)
    m = len(S)
    i = np.arange(1, m + 1, dtype=np.int64)
    return float(top(i, S - i, G, m).max()), float(bottom(i, S - i, G, m).min())


def blocked(i, j, G, m, x):
    """Does hit i after j misses end the walk?  (the comparison of the contract, in f64)"""
    return top(i, j, G, m) >= x if x > 0 else bottom(i, j, G, m) <= x


def tail_exact(G, m, x):
    """P(maxP >= x) for x > 0, P(minP <= x) for x < 0, 1 for x == 0, as a Fraction.  N(i, j): the unblocked prefixes with i hits
    and j misses; a blocked hit at step t = i + j out of (i, j) ends comb(G - t - 1, m - i - 1) sets."""
    x = float(x)
    if x == 0:
        return Fraction(1)
    js = np.arange(G - m + 1, dtype=np.int64)
    if x > 0:                                                 # top grows with i and falls with j: nothing is blocked past the
        last = np.flatnonzero(blocked(m, js, G, m, x))        # last j that blocks hit m, so those columns need no count
        if len(last) == 0:
            return Fraction(0)
        js = js[:last[-1] + 1]
    W = len(js)
    prev = [1] * W                                            # N(0, j)
    count = 0
    for i in range(1, m + 1):
        blk = blocked(i, js, G, m, x)
        if x < 0 and not blk.any():                           # bottom grows with i: no later hit is blocked either
            break
        blk = blk.tolist()
        n, k = G - i, m - i                                   # the sets a blocked hit out of (i - 1, j) ends: comb(n - j, k)
        c = comb(n, k)
        cur, run = [0] * W, 0
        for j in range(W):
            if blk[j]:
                if prev[j]:
                    count += prev[j] * c
            else:
                run += prev[j]
            cur[j] = run
            if j < G - m:
                c = c * (n - j - k) // (n - j)                # comb(n - j - 1, k), exactly
        if not run:
            break
        prev = cur
    return Fraction(count, comb(G, m))


def tail_enumerated(G, m):
    """Every attainable (maxP, minP) with the exact share of m-subsets at or beyond it: two dicts x -> Fraction."""
    tops, bots = [], []
    for S in combinations(range(1, G + 1), m):
        a, b = max_min(S, G)
        tops.append(a)
        bots.append(b)
    tops, bots, n = np.asarray(tops), np.asarray(bots), comb(G, m)
    return ({float(x): Fraction(int((tops >= x).sum()), n) for x in np.unique(tops)},
            {float(x): Fraction(int((bots <= x).sum()), n) for x in np.unique(bots)})


def reg_count(m):
    """R: hit indices per lane, the smallest power of two with 64 R >= m + 1."""
    R = 1
    while LANES * R < m + 1:
        R *= 2
    return R


def stair(G, m, x):
    """J[i'], i' in 1 .. m, of the walk the library runs: hit i' after j' misses is blocked iff j' <= J[i'] (-1: never).  x > 0:
    top(i', j') >= x.  x < 0, the mirrored set: bottom(m - i' + 1, G - m - j') <= x."""
    ip = np.arange(1, m + 1, dtype=np.int64)[:, None]
    jp = np.arange(G - m + 1, dtype=np.int64)[None, :]
    blk = top(ip, jp, G, m) >= x if x > 0 else bottom(m - ip + 1, G - m - jp, G, m) <= x
    assert (blk[:, :-1] >= blk[:, 1:]).all()                 # a prefix in j'
    return blk.sum(axis=1) - 1


def tail_f64(G, m, x):
    """The library's arithmetic: lane l of 64 holds the hit indices [l R, (l + 1) R); step t multiplies by inv = fl(1 / (G - t))."""
    x = float(x)
    if x == 0:
        return 1.0
    if m > MAX_SIZE:
        return float("nan")
    R = reg_count(m)
    idx = np.arange(LANES * R, dtype=np.int64).reshape(LANES, R)
    J = stair(G, m, x)
    B = np.full(LANES * R, -1, dtype=np.int64)
    B[:m] = J + np.arange(m)                                  # the hit out of index i is blocked while t <= J[i + 1] + i
    B = B.reshape(LANES, R)
    a = np.zeros((LANES, R), dtype=np.float64)
    a[0, 0] = 1.0
    hc = (m - idx).astype(np.float64)
    tl = np.zeros(LANES, dtype=np.float64)
    for t in range(int(B.max()) + 1):
        inv = np.float64(1.0) / np.float64(G - t)
        mc = (G - m - t + idx).astype(np.float64)
        h = a * (hc * inv)
        c = np.where(t > B, h, 0.0)
        for r in range(R - 1, -1, -1):
            tl = tl + (h[:, r] - c[:, r])
        cin = np.concatenate([[0.0], c[:-1, R - 1]])
        a = a * (mc * inv) + np.concatenate([cin[:, None], c[:, :R - 1]], axis=1)
    d = 32
    while d >= 1:                                             # lane l adds lane l ^ d
        tl = tl + tl[np.arange(LANES) ^ d]
        d //= 2
    return float(tl[0])


def rel_bound(G):
    return 4.0 * G * 2.0 ** -52
