"""The block solver of include/gficf_spectral.h restated in numpy: block Krylov in f64 with block size b = ndim, two projection
passes against [q0 V], two Gram passes within the block, Rayleigh-Ritz by ``eigh``, thick restart with keep = ndim + 2 (the
two extra ones chosen by the header's rule where a restarted cycle holds a single block).

A statement of the METHOD, not a port of libgficf_spectral.so: the sums run in numpy's order and the small problem goes through
``eigh`` where the library sweeps Jacobi rotations, so no bit is expected to agree.  What it is for: it shows that a case is
solvable by the method within max_restarts, and it bounds the restarts the device may take (tests/test_spectral_ndim_gpu.py
allows twice its count plus two).  Vectors are checked against ``eigh`` of the dense operator (tests/helpers/spectral_np.py), never
against this module.

``narrow_last_block``: the rule the header stated before this module existed ("the last block may be narrower than b" whenever
the basis fills up).  With it a cycle that is capped by m discards columns of a remainder, S V - V H is no longer confined to
the last block's remainder, and the iteration stalls (tests/test_spectral_cpu.py pins two such cases).  Without it (the rule of
the header now) a cycle capped by m ends at its last FULL block, and the narrower block is taken only when the basis is capped
by N - 1, where the complement of q0 is exhausted and the columns left out are dependent anyway."""
import numpy as np
import scipy.sparse as sp

EPS23 = 2.0 ** (-52.0 * 2.0 / 3.0)


def _gram_schmidt(G, bw, first, nb):
    """T (b x b) with W T orthonormal for G = W' W, column by column in the G inner product; the header's drop rules.  Returns
    (T, alive): alive[j] for j < bw."""
    b = G.shape[0]
    T = np.zeros((b, b))
    alive = np.zeros(bw, dtype=bool)
    for j in range(b):
        gjj = G[j, j]
        dead = j >= bw
        if not dead:
            dead = not (gjj > 1e-24 * (nb[j] + gjj)) if first else not (gjj > 0.0)
        if not dead:
            t = np.zeros(b)
            t[j] = 1.0
            for i in range(j):
                t -= (T[:, i] @ G[:, j]) * T[:, i]
            n2 = float(t @ (G @ t))
            dead = not (n2 > 1e-12 * gjj)
            if not dead:
                T[:, j] = t / np.sqrt(n2)
        if j < bw:
            alive[j] = not dead
    return T, alive


def solve(P, ndim, start, tol, m, max_restarts, narrow_last_block=False):
    """(values, vectors, residuals, restarts, multiplications, converged) of the header's method on the symmetric graph P."""
    A = sp.csr_matrix(P).astype(np.float64)
    N, b = A.shape[0], int(ndim)
    assert N > b >= 1 and m >= 2 * b + 2
    d = np.asarray(A.sum(axis=1)).ravel()
    assert (d > 0).all()
    dis = 1.0 / np.sqrt(d)
    S = sp.diags(dis) @ A @ sp.diags(dis)
    q0 = np.sqrt(d)
    q0 /= np.linalg.norm(q0)
    mc = min(int(m), N - 1)
    V = np.zeros((N, mc))
    flags = np.zeros(mc, dtype=bool)
    H = np.zeros((mc, mc + b))
    state = {"mults": 0}

    def mul(X):
        state["mults"] += 1
        return S @ X

    def project(W, nc):
        """W against q0 and the first nc columns of V, twice: (W, the summed coefficients on V, what the projection took out)."""
        Q = np.concatenate([V[:, :nc], q0[:, None]], axis=1)
        coef, nb = np.zeros((nc, b)), np.zeros(b)
        for _ in range(2):
            c = Q.T @ W
            W = W - Q @ c
            coef += c[:nc]
            nb += (c * c).sum(axis=0)
        return W, coef, nb

    def orth(W, bw, nb):
        alive = None
        for first in (True, False):
            T, alive = _gram_schmidt(W.T @ W, bw, first, nb)
            W = W @ T
        return W, alive

    def take(W, alive, col0, bw):
        """the block's first bw columns become columns col0 .. of V; the next multiplicand (columns >= bw are zero)"""
        V[:, col0:col0 + bw] = W[:, :bw]
        flags[col0:col0 + bw] = alive
        X = np.zeros((N, b))
        X[:, :bw] = W[:, :bw]
        return X

    W, _, nb = project(np.array(start, dtype=np.float64), 0)
    bw = min(b, mc)
    W, alive = orth(W, bw, nb)
    X = take(W, alive, 0, bw)
    c0, nc, keep, restarts, converged = 0, bw, 0, 0, False
    kept = np.zeros(0)
    while True:
        # ---- one cycle
        while True:
            W, coef, nb = project(mul(X), nc)
            H[:nc, c0:c0 + b] = coef
            if nc == mc:
                break
            if not narrow_last_block and mc < N - 1 and mc - nc < b:
                break                                           # capped by m: the cycle ends at its last full block
            bwn = min(b, mc - nc)
            Wn, alive = orth(W, bwn, nb)
            X = take(Wn, alive, nc, bwn)
            c0, bw, nc = nc, bwn, nc + bwn
        me = nc
        G = W.T @ W
        # ---- Rayleigh-Ritz on the live columns
        live = [j for j in range(me) if j < keep or flags[j]]
        n = len(live)
        if n < b:
            raise ValueError(f"the start block spans {n} directions outside the trivial eigenvector, ndim = {b} asked for")
        Hs = np.zeros((n, n))
        for x, i in enumerate(live):
            for y in range(x, n):
                j = live[y]
                h = (kept[i] if i == j else 0.0) if j < keep else H[i, j]
                Hs[x, y] = Hs[y, x] = h
        ev, Z = np.linalg.eigh(Hs)
        ev, Z = ev[::-1], Z[:, ::-1]
        Zfull = np.zeros((me, n))
        Zfull[live] = Z
        Zl = Zfull[me - bw:me, :b]
        theta = ev[:b].copy()
        est = np.sqrt(np.maximum(np.einsum("xl,xy,yl->l", Zl, G[:bw, :bw], Zl), 0.0))
        ok_est = bool((est <= tol * np.maximum(np.abs(theta), EPS23)).all())
        kp = min(b + 2, n)
        can_restart = restarts < max_restarts and kp < me
        if ok_est or not can_restart:
            Xf = V[:, :me] @ Zfull[:, :b]
            for c in range(b):
                if Xf[int(np.argmax(np.abs(Xf[:, c]))), c] < 0:
                    Xf[:, c] = -Xf[:, c]
            res = np.linalg.norm(mul(Xf) - Xf * theta[None, :], axis=0)
            converged = bool((res <= tol * np.maximum(np.abs(theta), EPS23)).all())
            if converged or not can_restart:
                return theta, Xf, res, restarts, state["mults"], converged
        # ---- thick restart
        restarts += 1
        sel = list(range(kp))
        if keep > 0 and n > kp and mc - kp < 2 * b:
            # one block per restarted cycle: the extra kept vectors are the Ritz vectors that carry most of the last leading b
            carried = (Zfull[:b, b:] ** 2).sum(axis=0)
            sel = list(range(b)) + sorted((b + np.argsort(-carried, kind="stable")[:kp - b]).tolist())
        V[:, :kp] = V[:, :me] @ Zfull[:, sel]
        T = np.zeros((b, b))
        T[:bw] = Zl
        W = W @ T
        keep, kept = kp, ev[sel].copy()
        W, _, nb = project(W, keep)
        bw = min(b, mc - keep)
        W, alive = orth(W, bw, nb)
        X = take(W, alive, keep, bw)
        c0, nc = keep, keep + bw
