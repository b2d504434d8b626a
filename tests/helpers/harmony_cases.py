"""The inputs the Harmony tests share: separated blobs with batch shifts at the shapes where the kernels can go wrong, the port's
own state at every stage (computed once a case, never changed), and the rounding bounds the comparisons allow."""
from __future__ import annotations

import functools

import numpy as np

from . import harmony_np as hp

U = hp.U
C = 4.0          # the constant of every summation bound: c n 2^-53 sum |terms|

# name: N, K, d, levels per variable, levels drawn from (the last level of "empty" stays without cells), n_blocks, theta
CASES = {
    # fewer cells than blocks (13 of the 20 blocks are empty)
    "n7": dict(N=7, K=2, d=2, nlev=(2,), n_blocks=20, theta=0.5),
    # ragged blocks of 4 and 3; one cluster, one column, one level
    "n61": dict(N=61, K=1, d=1, nlev=(1,), n_blocks=17, theta=2.0),
    # two variables, 64 clusters
    "v2": dict(N=600, K=64, d=50, nlev=(2, 3), n_blocks=3, theta=2.0),
    # 65 clusters (17 groups of four centroids, the last one holding a single one), the widest rows, 64 levels, the last one empty
    "b64": dict(N=600, K=65, d=128, nlev=(64,), empty=True, n_blocks=2, theta=1.0),
    # two variables of 32 levels: 1024 pair bins
    "b64v2": dict(N=600, K=2, d=2, nlev=(32, 32), n_blocks=2, theta=1.0),
    # more than four chunks of 1024 cells, a last chunk of 3; 100 clusters
    "n4099": dict(N=4099, K=100, d=50, nlev=(3,), n_blocks=2, theta=2.0),
}
SIGMA, LAMB, INIT_ITER = 0.1, 1.0, 3


def blobs(N, d, K, levels, B, seed):
    """K separated blobs on d columns, every level shifted."""
    r = np.random.default_rng(seed)
    cent = 4.0 * r.standard_normal((K, d)) + 1.0
    off = 0.3 * r.standard_normal((B, d))
    kind = np.arange(N) % K
    r.shuffle(kind)
    return cent[kind] + off[levels].sum(axis=0) + 0.05 * r.standard_normal((N, d)), kind


@functools.lru_cache(maxsize=None)
def case(name):
    """The case's inputs and the port's state after every stage."""
    c = dict(CASES[name])
    N, K, d = c["N"], c["K"], c["d"]
    r = np.random.default_rng(sum(map(ord, name)))
    var_start = np.concatenate([[0], np.cumsum(c["nlev"])]).astype(np.int32)
    B = int(var_start[-1])
    levels = np.stack([var_start[v] + r.integers(0, n - (1 if c.get("empty") else 0), N) for v, n in enumerate(c["nlev"])]).astype(np.int32)
    Z, kind = blobs(N, d, K, levels, B, 5 + N)
    theta, lamb = np.full(B, c["theta"]), np.full(B, LAMB)
    Zc, _ = hp.normalise(Z)
    first = np.array([np.flatnonzero(kind == k)[0] for k in range(K)])   # one cell of every blob starts a centroid
    Y0 = Zc[first].copy()
    Y, lab = hp.start(Zc, Y0, INIT_ITER)
    R, O, E = hp.assign(Zc, levels, B, Y, SIGMA)
    perm = r.permutation(N).astype(np.int32)
    R1, O1, E1, Y1 = hp.round_(Zc, levels, B, Y, R, O, E, theta, SIGMA, perm, c["n_blocks"])
    obj = hp.objective(Zc, levels, B, Y1, R1, O1, E1, theta, SIGMA)
    Zcorr, W, flat, cond = hp.correct(Z, levels, B, R1, lamb)
    out = dict(c, name=name, var_start=var_start, B=B, V=len(c["nlev"]), levels=levels, Z=Z, Zc=Zc, Y0=Y0, Y=Y, lab=lab, R=R, O=O, E=E, perm=perm,
               theta_b=theta, lamb_b=lamb, R1=R1, O1=O1, E1=E1, Y1=Y1, obj=obj, Zcorr=Zcorr, W=W, flat=flat, cond=cond)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ------------------------------------------------------------------ bounds (derived)
def dist_bound(Y, Zc):
    """dist = 2 (1 - y . z): a dot product of d terms in another order, then two more roundings of values up to 4."""
    d = Zc.shape[1]
    return 2.0 * (C * d * U * (np.abs(Y) @ np.abs(Zc).T)) + C * 2 * U * 4.0


def soft_rel_bound(dD, sigma, K):
    """Relative error of a normalised R entry when every dist of its column is off by at most dD: exp turns an absolute error
    x of its argument into a relative one (numerator and denominator: 2 dD / sigma each way), plus the K-term sum, the division
    and the exponentials' own roundings."""
    return 4.0 * dD / sigma + C * (K + 4) * U


def _centroid_ds(Wt, Zc):
    """s = Wt Zc, its norm, and the bound of every component of s: N terms in another order."""
    s = Wt @ Zc
    return s, np.sqrt((s * s).sum(axis=1)), C * Zc.shape[0] * U * (np.abs(Wt) @ np.abs(Zc))


def centroid_bound(Wt, Zc):
    """Components of Y = s / |s|: |dY_j| <= (ds_j + |ds|) / |s| (the norm moves by at most |ds|), and the division's rounding."""
    s, n, ds = _centroid_ds(Wt, Zc)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n[:, None] > 0, (ds + np.sqrt((ds * ds).sum(axis=1))[:, None]) / n[:, None] + C * 4 * U, 0.0)


def centroid_dist_shift(Wt, Zc):
    """What dist = 2 (1 - y . z), |z| = 1, moves by when Y does: 2 |dY| <= 4 |ds| / |s|, the largest over the centroids."""
    s, n, ds = _centroid_ds(Wt, Zc)
    return float(np.max(4.0 * np.sqrt((ds * ds).sum(axis=1))[n > 0] / n[n > 0] + C * 8 * U)) if (n > 0).any() else 0.0


def round_rel_bound(c, dD):
    """Relative error of R after a round of n non-empty blocks, by recursion over the blocks: a block's R carries the error of
    its exponentials and of V powers of (E + 1) / (O + 1), whose error is the bookkeeping's (sums of N terms and two additions a
    block) plus that of the R of the blocks before, amplified by at most amp = 1 + max O where a block holds most of a level."""
    N, K, V = c["N"], c["K"], c["V"]
    if K == 1:
        return 0.0                                             # R = e / e = 1 exactly, whatever e is
    th = float(np.max(c["theta_b"]))
    amp = 1.0 + float(np.max(c["O"]))
    base = soft_rel_bound(dD, SIGMA, K) + C * V * (th + 4) * U * (1.0 + th * float(np.abs(np.log((c["E"] + 1) / (c["O"] + 1))).max()))
    e, blocks = 0.0, min(c["n_blocks"], N)
    for j in range(1, blocks + 1):
        e = max(e, base + 2.0 * V * th * amp * (C * (N + 2 * j) * U + e))
    return e
