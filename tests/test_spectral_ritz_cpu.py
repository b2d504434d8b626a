"""No GPU: the host mathematics of the spectral solve (gficf_amd/csrc/spectral_ritz.h: the Rayleigh-Ritz step, the final rotation,
the restart choice) through tests/helpers/spectral_ritz_probe.cpp, built with the host C++ compiler and bound with ctypes.

Floating-point bound.  Cyclic Jacobi and ``eigh`` are both backward stable to a small multiple of n eps |H|; over every case of
this file the largest of max|ev - eigh| / |H|_2, max|Z'Z - I| and max|H Z - Z diag(ev)| / |H|_2 was measured at 1.83e-14 on an
x86-64 CPU with g++ -O2 (the first 1.83e-14, the second 1.82e-14, the third 6.6e-15; n up to 64).  Allowed: 16 times that,
BOUND = 2.93e-13: only the last bits depend on the compiler.  Every case prints its three figures before it asserts."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.helpers import spectral_block_np as sb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED = 1.83e-14
BOUND = 16 * MEASURED
WIDTHS = (1, 2, 3, 8)
_dp, _ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(a):
    return a.ctypes.data_as(_ip)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("spectral_ritz") / "libspectral_ritz_probe.so")
    cmd = [cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-I", os.path.join(ROOT, "gficf_amd", "csrc"),
           os.path.join(ROOT, "tests", "helpers", "spectral_ritz_probe.cpp"), "-o", so]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    L = ctypes.CDLL(so)
    ci, cd = ctypes.c_int, ctypes.c_double
    L.probe_sp_ritz.restype, L.probe_sp_ritz.argtypes = ci, [ci] * 5 + [_dp, _dp, _ip, _dp, cd, _ip, _dp, _dp, _dp, _ip]
    L.probe_sp_final_rotation.restype, L.probe_sp_final_rotation.argtypes = None, [ci, ci, ci, _dp, _dp]
    L.probe_sp_restart_choice.restype, L.probe_sp_restart_choice.argtypes = ci, [ci] * 6 + [_dp, _dp, _ip, _dp, _dp, _dp]
    return L


SENTINEL = -7.25


def ritz(L, me, keep, bw, b, H, flags, G, tol, kept=None, ldh=None, fill=np.nan):
    """The Ritz step on the me x me matrix H: only what the header may read of it is handed over (the upper triangle of the
    columns >= keep; everything else of hH is ``fill``).  Returns (n, live, ev, Zfull, theta, pass) and checks the guard cells."""
    ldh = me + 3 if ldh is None else ldh
    hH = np.full((me, ldh), fill)                               # hH[j, i]: element (i, j) at i + ldh j
    for j in range(keep, me):
        hH[j, :j + 1] = H[:j + 1, j]
    kept = np.zeros(0) if kept is None else np.ascontiguousarray(kept, dtype=np.float64)
    flags = np.ascontiguousarray(flags, dtype=np.int32)
    G = np.ascontiguousarray(G, dtype=np.float64)
    live = np.full(me + 1, -1, dtype=np.int32)
    ev, Z, theta = np.full(me + 1, SENTINEL), np.full(me * me + 1, SENTINEL), np.full(b + 1, SENTINEL)
    ok = np.full(2, -1, dtype=np.int32)
    n = L.probe_sp_ritz(me, keep, bw, b, ldh, _d(kept), _d(hH), _i(flags), _d(G), float(tol), _i(live), _d(ev), _d(Z), _d(theta), _i(ok))
    assert live[me] == -1 and ev[me] == SENTINEL and Z[me * me] == SENTINEL and theta[b] == SENTINEL and ok[1] == -1
    if n < b:
        assert (ev == SENTINEL).all() and (Z == SENTINEL).all() and (theta == SENTINEL).all() and ok[0] == -1
        return n, live[:n].copy(), None, None, None, None
    assert (Z[me * n:] == SENTINEL).all() and (ev[n:] == SENTINEL).all() and ok[0] in (0, 1)
    return n, live[:n].copy(), ev[:n].copy(), Z[:me * n].reshape(me, n).copy(), theta[:b].copy(), bool(ok[0])


def restart_choice(L, Zfull, ev, keep, bw, b, mc):
    me, n = Zfull.shape
    sel = np.full(b + 3, -1, dtype=np.int32)
    up, zl, kept = np.full(me * (b + 2) + 1, SENTINEL), np.full(b * b + 1, SENTINEL), np.full(b + 3, SENTINEL)
    kp = L.probe_sp_restart_choice(n, me, keep, bw, b, mc, _d(np.ascontiguousarray(Zfull)), _d(np.ascontiguousarray(ev)), _i(sel), _d(up), _d(zl), _d(kept))
    assert kp == min(b + 2, n)
    assert (sel[kp:] == -1).all() and (up[me * kp:] == SENTINEL).all() and zl[b * b] == SENTINEL and (kept[kp:] == SENTINEL).all()
    return kp, sel[:kp].copy(), up[:me * kp].reshape(me, kp).copy(), zl[:b * b].reshape(b, b).copy(), kept[:kp].copy()


def sizes(b, lo=None):
    """me from b up to 64: next to b, around the smallest basis 2 b + 2, odd and even, 64"""
    lo = b if lo is None else lo
    return sorted(set(v for v in (b, b + 1, b + 2, b + 3, 2 * b + 2, 2 * b + 3, 3 * b + 1, 17, 32, 33, 64) if lo <= v <= 64))


def sym(rng, n, scale=1.0):
    A = rng.standard_normal((n, n))
    return scale * (A + A.T) / 2


def gram(rng, b):
    A = rng.standard_normal((b + 2, b))
    return A.T @ A


def projected(H, keep, kept):
    """What the Ritz step decomposes: diag(kept) on the kept columns and zero off it there, the upper triangle of H elsewhere, mirrored"""
    A = np.triu(H)
    A[:, :keep] = 0.0
    A[:keep, :keep] = np.diag(kept)
    return A + np.triu(A, 1).T


DEVIATION = {"ev": 0.0, "orth": 0.0, "pairs": 0.0}


def check_against_eigh(Hs, live, ev, Zfull):
    """ev, Zfull against eigh of Hs (the projected matrix on the live columns): the three floating-point comparisons"""
    n = len(live)
    Z = Zfull[live]
    norm = max(np.linalg.norm(Hs, 2), np.finfo(float).tiny)
    w = np.linalg.eigh(Hs)[0][::-1]
    dev = {"ev": np.abs(ev - w).max() / norm, "orth": np.abs(Z.T @ Z - np.eye(n)).max(), "pairs": np.abs(Hs @ Z - Z * ev[None, :]).max() / norm}
    for k, v in dev.items():
        DEVIATION[k] = max(DEVIATION[k], float(v))
    print(f"n {n}: {dev}, largest so far {DEVIATION}")
    assert (np.diff(ev) <= 0).all()
    assert max(dev.values()) <= BOUND, dev
    dead = np.setdiff1d(np.arange(Zfull.shape[0]), live)
    assert (Zfull[dead] == 0.0).all() and not np.signbit(Zfull[dead]).any()


# ------------------------------------------------------------------------------------------------ case 1: a first cycle
@pytest.mark.parametrize("b", WIDTHS)
def test_first_cycle_equals_eigh_and_reads_the_upper_triangle_only(probe, b):
    rng = np.random.default_rng(100 + b)
    for me in sizes(b):
        for scale in (1.0, 1e-3):
            H = sym(rng, me, scale)
            n, live, ev, Zfull, theta, _ = ritz(probe, me, 0, min(b, me), b, H, np.ones(me), gram(rng, b), 1e-4)      # below the diagonal: NaN
            assert n == me and live.tolist() == list(range(me))
            check_against_eigh(H, live, ev, Zfull)
            assert np.array_equal(theta, ev[:b])
            up = np.full(me * b + 1, SENTINEL)
            probe.probe_sp_final_rotation(me, n, b, _d(np.ascontiguousarray(Zfull)), _d(up))
            assert up[me * b] == SENTINEL and np.array_equal(up[:me * b].reshape(me, b), Zfull[:, :b])                # me x b row-major


# ------------------------------------------------------------------------------------------------ case 2: dropped columns
@pytest.mark.parametrize("b", WIDTHS)
def test_dropped_columns_have_zero_rows(probe, b):
    rng = np.random.default_rng(200 + b)
    for me in sizes(b, b + 1):
        for keep in (0, b + 2):
            if keep >= me:
                continue
            H = sym(rng, me)
            kept = np.sort(rng.uniform(0.5, 1.0, keep))[::-1]
            flags = np.ones(me, dtype=np.int32)
            free = np.arange(keep, me)
            drop = rng.choice(free, size=min(len(free), max(1, (me - max(keep, b)) // 2)), replace=False)
            if me - len(drop) < b:
                drop = drop[:me - b]
            flags[drop] = 0
            flags[:keep] = 0                                    # a kept column is live whatever its flag says
            live_want = [j for j in range(me) if j < keep or flags[j]]
            n, live, ev, Zfull, theta, _ = ritz(probe, me, keep, min(b, me - keep), b, H, flags, gram(rng, b), 1e-4, kept)
            assert n == len(live_want) >= b and live.tolist() == live_want
            check_against_eigh(projected(H, keep, kept)[np.ix_(live, live)], live, ev, Zfull)
            assert np.array_equal(theta, ev[:b])


@pytest.mark.parametrize("b", WIDTHS)
def test_fewer_than_b_live_columns_are_reported_and_nothing_is_written(probe, b):
    rng = np.random.default_rng(300 + b)
    for me in sizes(b)[:6]:
        for n_live in sorted(set((0, b - 1))):
            flags = np.zeros(me, dtype=np.int32)
            flags[rng.choice(me, size=n_live, replace=False)] = 1
            n, live, ev, _, _, _ = ritz(probe, me, 0, min(b, me), b, sym(rng, me), flags, gram(rng, b), 1e-4)  # ritz() checks the outputs untouched
            assert n == n_live < b and ev is None and live.tolist() == np.flatnonzero(flags).tolist()


# ------------------------------------------------------------------------------------------------ case 3: a restarted cycle
@pytest.mark.parametrize("b", WIDTHS)
def test_restarted_cycle_is_the_arrowhead_matrix(probe, b):
    rng = np.random.default_rng(400 + b)
    keep = b + 2
    for me in sizes(b, keep + 1):
        H = sym(rng, me)
        kept = np.sort(rng.uniform(0.5, 1.0, keep))[::-1]
        n, live, ev, Zfull, theta, _ = ritz(probe, me, keep, min(b, me - keep), b, H, np.ones(me), gram(rng, b), 1e-4, kept)   # columns < keep of hH: NaN
        A = projected(H, keep, kept)
        assert n == me and np.array_equal(A[:keep, :keep], np.diag(kept))
        check_against_eigh(A, live, ev, Zfull)
        assert np.array_equal(theta, ev[:b])


# ------------------------------------------------------------------------------------------------ case 4: the estimate
def np_estimate(Zfull, ev, G, me, bw, b):
    """tests/helpers/spectral_block_np.py, the lines that form est and its threshold; returns est / max(|theta|, eps^(2/3))"""
    Zl = Zfull[me - bw:me, :b]
    theta = ev[:b].copy()
    est = np.sqrt(np.maximum(np.einsum("xl,xy,yl->l", Zl, G[:bw, :bw], Zl), 0.0))
    return est / np.maximum(np.abs(theta), sb.EPS23)


@pytest.mark.parametrize("b", WIDTHS)
def test_estimate_verdict_equals_the_numpy_expression(probe, b):
    rng = np.random.default_rng(500 + b)
    seen = set()
    for me in sizes(b):
        for zero in (False, True)[:2 if me == b else 1]:        # H = 0 (Z = I, so at me = b): every theta is 0, the threshold is tol eps^(2/3)
            H = np.zeros((me, me)) if zero else sym(rng, me)
            G, bw = gram(rng, b), min(b, me)
            _, _, ev, Zfull, _, _ = ritz(probe, me, 0, bw, b, H, np.ones(me), G, 1.0)
            ratio = np_estimate(Zfull, ev, G, me, bw, b)        # pair l passes when ratio[l] <= tol
            assert (ratio > 0).all() and (not zero or (ev == 0).all())
            s = np.sort(ratio)
            tols = [s[-1] * 10, s[0] / 10] + [np.sqrt(s[k] * s[k + 1]) for k in range(b - 1) if s[k + 1] >= 100 * s[k]]
            for tol in tols:
                assert (np.maximum(ratio / tol, tol / ratio) >= 10 * (1 - 1e-12)).all()      # every estimate a factor 10 from its threshold
                want = bool((ratio <= tol).all())
                got = ritz(probe, me, 0, bw, b, H, np.ones(me), G, tol)[5]
                assert got == want
                seen.add(want)
    assert seen == {True, False}


# ------------------------------------------------------------------------------------------------ case 5: the restart choice
def np_choice(Zfull, ev, keep, b, mc):
    """tests/helpers/spectral_block_np.py, the lines that choose what a restart keeps; (sel, carried or None)"""
    n = Zfull.shape[1]
    kp = min(b + 2, n)
    sel, carried = list(range(kp)), None
    if keep > 0 and n > kp and mc - kp < 2 * b:
        carried = (Zfull[:b, b:] ** 2).sum(axis=0)
        sel = list(range(b)) + sorted((b + np.argsort(-carried, kind="stable")[:kp - b]).tolist())
    return sel, carried


def check_choice(probe, Zfull, ev, keep, bw, b, mc, want_rule, distinct=True):
    me, n = Zfull.shape
    sel_want, carried = np_choice(Zfull, ev, keep, b, mc)
    assert (carried is not None) == want_rule
    if carried is not None and distinct:
        assert np.diff(np.sort(carried)).min() > 1e-9           # no two carried weights that a summation order could swap
    kp, sel, up, zl, kept = restart_choice(probe, Zfull, ev, keep, bw, b, mc)
    assert sel.tolist() == sel_want and np.array_equal(kept, ev[sel_want])
    assert np.array_equal(up, Zfull[:, sel_want])               # me x kp row-major
    assert np.array_equal(zl[:bw], Zfull[me - bw:me, :b]) and (zl[bw:] == 0.0).all()
    return sel


@pytest.mark.parametrize("b", WIDTHS)
def test_restart_choice_identity_and_carried_weight(probe, b):
    rng = np.random.default_rng(600 + b)
    keep = b + 2
    ruled = 0
    for me in sizes(b, keep + 1):
        for drop in (False, True):
            flags = np.ones(me, dtype=np.int32)
            if drop and me - keep > b:
                flags[me - 1 - b] = 0
            kept = np.sort(rng.uniform(0.5, 1.0, keep))[::-1]
            bw = min(b, me - keep)
            n, _, ev, Zfull, _, _ = ritz(probe, me, keep, bw, b, sym(rng, me), flags, gram(rng, b), 1e-4, kept)
            rule = n > keep and me - keep < 2 * b                # mc = me: a restarted cycle of a single block
            sel = check_choice(probe, Zfull, ev, keep, bw, b, me, rule)
            ruled += rule and sel.tolist() != list(range(keep))
            check_choice(probe, Zfull, ev, keep, bw, b, keep + 2 * b, False)      # room for two blocks: the leading kp
            check_choice(probe, Zfull, ev, 0, bw, b, me, False)                   # the first restart: the leading kp
    assert ruled >= 1                                            # the rule chose something other than the leading kp at least once


def test_restart_choice_takes_the_lowest_index_on_ties(probe):
    b, me, keep = 2, 7, 4
    Zfull = np.full((me, me), 0.5)
    Zfull[2:, ::2] = -0.5
    Zfull[:2, 2:] = np.array([[0.5, 0.5, -0.5, 0.5, 0.0], [0.0, 0.5, 0.5, -0.5, 0.0]])     # carried: .25, .5, .5, .5, 0
    ev = np.linspace(1.0, 0.4, me)
    sel = check_choice(probe, Zfull, ev, keep, 2, b, me, True, distinct=False)
    assert sel.tolist() == [0, 1, 3, 4]


# ------------------------------------------------------------------------------------------------ case 6: nothing to restart with
@pytest.mark.parametrize("b", WIDTHS)
def test_kp_equals_n_leaves_nothing_to_restart_with(probe, b):
    rng = np.random.default_rng(700 + b)
    for me in range(b, b + 3):
        n, _, ev, Zfull, _, _ = ritz(probe, me, 0, min(b, me), b, sym(rng, me), np.ones(me), gram(rng, b), 1e-4)
        kp, sel, up, _, kept = restart_choice(probe, Zfull, ev, 0, min(b, me), b, me)
        assert kp == n == me and not kp < me                    # the caller's can_restart: restarts left and kp < me
        assert sel.tolist() == list(range(n)) and np.array_equal(up, Zfull) and np.array_equal(kept, ev)

