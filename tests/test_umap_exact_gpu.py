"""GPU: the layout sweep of libgficf_umap.so, bit for bit.

include/gficf_umap.h states the sweep operation by operation, umap.hip is built without fused multiply-adds for that reason, and
on the t-UMAP curve (a == b == 1) the force law of csrc/umap_force.h holds nothing but IEEE operations: subtraction, multiplication,
addition, a correctly rounded division, minimum and maximum.  tests/helpers/umap_np.layout(dtype=float32) evaluates the same
operations in the same order, so the two must agree in every bit of every coordinate.  These tests ask for that: np.array_equal
on the uint32 views, no tolerance, no vertex left out.

The graphs (tests/helpers/umap_cases.py) are crafted for the places where the kernel changes its path: rows that end a group
round ragged, both sides of the hub threshold, negative-sample rates around the 8 lanes of a group and the 64 of a wave (a second
round of the sample loop on the wave path needs a rate above 64), more hubs than the waves that share the hub list, and starting
positions that coincide (d2 == 0 in both forces).  tests/test_umap_cpu.py asserts, without a GPU, that the schedule really takes
the sweep to those places in the tested epochs and that the float64 port would fail every one of these comparisons.

MEASURED_EXACT: per case the vertices compared (all of them) and the largest coordinate deviation between the port's float32 and
float64 runs, which is what a tolerance test of that case would have had to forgive (``python -m tests.helpers.umap_cases``
prints the table; tests/test_umap_cpu.py asserts that it is above 0 beyond epoch 0).

The (1.8956, 0.8006) curve calls powf, whose bits are the device library's own; for it the sharp statement is that the wave path
and the group path give the same bits: a row padded beyond the hub threshold with entries that are never due against the same
row without them."""
import numpy as np
import pytest

import gficf_amd
from tests.helpers import umap_cases as uc

pytestmark = pytest.mark.gpu

# (graph, epochs of 200, negative_sample_rate): (vertices compared, |port f32 - port f64|)
MEASURED_EXACT = {
    ('seams', '100-101', 0): (300, 2.518e-06),
    ('seams', '100-101', 1): (300, 5.117e-06),
    ('seams', '100-101', 5): (300, 2.000e+00),
    ('seams', '100-101', 7): (300, 3.218e+00),
    ('seams', '100-101', 8): (300, 3.219e+00),
    ('seams', '100-101', 9): (300, 3.219e+00),
    ('seams', '100-101', 16): (300, 5.440e-03),
    ('seams', '100-101', 17): (300, 5.648e-03),
    ('seams', '100-101', 63): (300, 1.773e-03),
    ('seams', '100-101', 64): (300, 1.804e-03),
    ('seams', '100-101', 65): (300, 7.202e-03),
    ('seams', '100-101', 130): (300, 1.639e-02),
    ('seams', '0-1', 5): (300, 4.768e-07),
    ('seams', '100-103', 5): (300, 3.681e+00),
    ('many_hubs', '100-102', 5): (1100, 6.367e+00),
    ('rand', '0-1', 5): (257, 4.736e-07),
    ('rand', '100-101', 5): (257, 5.424e-05),
    ('rand', '0-3', 5): (257, 6.416e-03),
    ('hub', '0-1', 5): (2001, 4.697e-07),
    ('hub', '100-101', 5): (2001, 4.367e-04),
    ('hub', '0-3', 5): (2001, 2.888e-03),
    ('crafted', '100-101', 5): (257, 2.770e-04),
}


def _bits(Y):
    Y = np.ascontiguousarray(Y)
    assert Y.dtype == np.float32
    return Y.view(np.uint32)


def _device(P, Y0, window, rate, ab="tumap"):
    a, b = uc.AB[ab]
    lo, hi = uc.WINDOWS[window]
    return gficf_amd.umap_layout(P, Y0, uc.LAYOUT_EPOCHS, a, b, negative_sample_rate=rate, seed=uc.LAYOUT_SEED, epoch_begin=lo, epoch_end=hi)


def test_measured_table_names_every_case():
    assert set(MEASURED_EXACT) == set(uc.exact_cases())


@pytest.mark.parametrize("case", uc.exact_cases(), ids=uc.exact_id)
def test_layout_equals_the_float32_port_in_bits(case):
    graph, window, rate = case
    P, Y0 = uc.exact_graph(graph)
    got = _device(P, Y0, window, rate)
    want = uc.exact_port(graph, window, rate, np.float32)
    differ = (_bits(got) != _bits(want)).any(axis=1)
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print(f"{uc.exact_id(case)}: {len(want)} vertices compared, {int(differ.sum())} differ, |device - port f32| = {err:.3e}, "
          f"port f32 / f64 = {MEASURED_EXACT[case][1]:.3e}")
    assert got.shape == want.shape == (P.shape[0], 2) and len(want) == MEASURED_EXACT[case][0]
    assert np.array_equal(_bits(got), _bits(want)), np.flatnonzero(differ)[:10]
    if uc.WINDOWS[window] == (0, 1):
        assert np.array_equal(_bits(got), _bits(np.asarray(Y0, dtype=np.float32)))     # no entry is due in epoch 0


@pytest.mark.parametrize("rate", uc.PADDED_RATES)
@pytest.mark.parametrize("L,pad", uc.PADDED)
@pytest.mark.parametrize("ab", list(uc.AB))
def test_wave_path_equals_group_path(ab, L, pad, rate):
    """Row v with L entries is walked by a group of 8 lanes; with ``pad`` more entries that are never due, by a whole wave."""
    P, Y0, v = uc.padded(L, pad)
    Q, _, _ = uc.padded(L, 0)
    wave, group = _device(P, Y0, uc.PADDED_WINDOW, rate, ab), _device(Q, Y0, uc.PADDED_WINDOW, rate, ab)
    start = np.asarray(Y0, dtype=np.float32)
    assert np.isfinite(wave).all() and (wave[v] != start[v]).any()                      # row v had work to do
    assert np.array_equal(_bits(wave), _bits(group)), np.flatnonzero((_bits(wave) != _bits(group)).any(axis=1))[:10]
