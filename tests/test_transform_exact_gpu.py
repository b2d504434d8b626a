"""GPU: the layout sweep and the initial positions of libgficf_transform.so, bit for bit.

include/gficf_transform.h states both operation by operation, transform.hip is built without fused multiply-adds, and on the
t-UMAP curve (a == b == 1) the force law of csrc/umap_force.h holds nothing but IEEE operations; k_tr_init is sums, products and
one correctly rounded division.  tests/helpers/transform_np.layout(dtype=float32) and init_positions evaluate the same operations
in the same order, so the device must agree with them in every bit: np.array_equal on the uint32 views, no tolerance, no cell
left out.

The cases (tests/helpers/transform_cases.py) are the recipe of layout_case("rand") at the k around the 8 lanes of a group (1, 7,
8, 9, 16, 17, 128), cut to M cells around the 8 cells of a workgroup (1, 7, 8, 9, 500), at negative-sample rates around a group
(0, 7, 8, 9, 17), over two epochs, so that the running position passes from one epoch to the next in registers.  A cell's
result depends on its row and on query_offset + i only, so the first M rows of the port's one run are the reference for M cells.
tests/test_transform_cpu.py asserts, without a GPU, that statement for the port, that the schedule reaches every kind of round in
the tested epochs, and that the float64 port would fail every one of these comparisons.

MEASURED_EXACT: per case the cells compared at M = 500 (all of them) and the largest coordinate deviation between the port's
float32 and float64 runs, which is what a tolerance test of that case would have had to forgive
(``python -m tests.helpers.transform_cases`` prints the table).

The (1.8956, 0.8006) curve calls powf, whose bits are the device library's own; for it the sharp statement stays that two query
blocks run with their offsets give the bits of the whole, here at k = 1, 8, 9 and 128."""
import numpy as np
import pytest

from tests.helpers import transform_cases as tc
from tests.helpers import transform_np as tn

pytestmark = pytest.mark.gpu

# (input, k, negative_sample_rate), epochs [30, 32) of 67: (cells compared, |port f32 - port f64|)
MEASURED_EXACT = {
    ('rand', 1, 0): (500, 3.615e-07),
    ('rand', 1, 7): (500, 9.714e-07),
    ('rand', 1, 8): (500, 2.168e-06),
    ('rand', 1, 9): (500, 1.430e-06),
    ('rand', 1, 17): (500, 1.185e-05),
    ('rand', 7, 0): (500, 5.827e-07),
    ('rand', 7, 7): (500, 2.217e-05),
    ('rand', 7, 8): (500, 2.854e-05),
    ('rand', 7, 9): (500, 2.841e-05),
    ('rand', 7, 17): (500, 1.953e-04),
    ('rand', 8, 0): (500, 7.892e-07),
    ('rand', 8, 7): (500, 5.631e-05),
    ('rand', 8, 8): (500, 6.984e-06),
    ('rand', 8, 9): (500, 1.570e-05),
    ('rand', 8, 17): (500, 1.112e-04),
    ('rand', 9, 0): (500, 1.274e-06),
    ('rand', 9, 7): (500, 1.331e-04),
    ('rand', 9, 8): (500, 1.678e-05),
    ('rand', 9, 9): (500, 4.458e-05),
    ('rand', 9, 17): (500, 1.851e-04),
    ('rand', 16, 0): (500, 1.124e-06),
    ('rand', 16, 7): (500, 3.894e-05),
    ('rand', 16, 8): (500, 3.032e-05),
    ('rand', 16, 9): (500, 5.786e-05),
    ('rand', 16, 17): (500, 3.856e-04),
    ('rand', 17, 0): (500, 1.350e-06),
    ('rand', 17, 7): (500, 1.401e-04),
    ('rand', 17, 8): (500, 2.840e-04),
    ('rand', 17, 9): (500, 1.652e-04),
    ('rand', 17, 17): (500, 8.763e-04),
    ('rand', 128, 0): (500, 9.603e-07),
    ('rand', 128, 7): (500, 1.422e-03),
    ('rand', 128, 8): (500, 1.932e-03),
    ('rand', 128, 9): (500, 3.502e-04),
    ('rand', 128, 17): (500, 9.351e-03),
    ('crafted', 8, 0): (500, 7.234e-07),
    ('crafted', 8, 7): (500, 5.631e-05),
}


def _bits(Y):
    Y = np.ascontiguousarray(Y)
    assert Y.dtype == np.float32
    return Y.view(np.uint32)


def _device(name, k, rate, first=0, stop=None, query_offset=0, ab="tumap"):
    idx, W, Yt, Y0 = tc.layout_case(name, k)
    a, b = tc.AB[ab]
    return tc.dev_layout(idx[first:stop], W[first:stop], Yt, Y0[first:stop], tc.LAYOUT_EPOCHS, a, b, **tc.exact_kw(rate, query_offset))


def test_measured_table_names_every_case():
    assert set(MEASURED_EXACT) == set(tc.exact_cases())


@pytest.mark.parametrize("case", tc.exact_cases(), ids=lambda c: "-".join(str(v) for v in c))
def test_layout_equals_the_float32_port_in_bits(case):
    name, k, rate = case
    want = tc.exact_port(name, k, rate, np.float32)
    for M in tc.EXACT_MS:
        got = _device(name, k, rate, stop=M)
        differ = (_bits(got) != _bits(want[:M])).any(axis=1)
        err = float(np.abs(got.astype(np.float64) - want[:M].astype(np.float64)).max())
        print(f"{case}, M = {M}: {M} cells compared, {int(differ.sum())} differ, |device - port f32| = {err:.3e}, "
              f"port f32 / f64 = {MEASURED_EXACT[case][1]:.3e}")
        assert got.shape == (M, 2) and np.array_equal(_bits(got), _bits(want[:M])), (M, np.flatnonzero(differ)[:10])
    assert len(want) == MEASURED_EXACT[case][0] == max(tc.EXACT_MS)


@pytest.mark.parametrize("k", tc.EXACT_KS)
@pytest.mark.parametrize("first,offset", tc.EXACT_OFFSETS)
def test_layout_with_a_query_offset_equals_the_float32_port_in_bits(first, offset, k):
    """Rows 250 .. 499 as the block they are of the whole batch, and the whole batch as a block far into a larger one (an offset
    beyond 2^32: the entry index of the sample key is a 64-bit product)."""
    got = _device("rand", k, 7, first=first, query_offset=offset)
    want = tc.exact_port("rand", k, 7, np.float32, first, offset)
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want))
    if first:
        assert np.array_equal(_bits(want), _bits(tc.exact_port("rand", k, 7, np.float32)[first:]))


@pytest.mark.parametrize("k", tc.INIT_KS)
def test_init_equals_the_port_in_bits(k):
    idx, W, Yt = tc.init_case(k)
    got, want = tc.dev_init(idx, W, Yt), tn.init_positions(idx, W, Yt)
    assert (W[tc.INIT_ZERO_ROW] == 0).all() and np.isfinite(want).all()                 # the plain mean is among the rows
    assert got.shape == want.shape == (len(idx), 2)
    assert np.array_equal(_bits(got), _bits(want)), np.flatnonzero((_bits(got) != _bits(want)).any(axis=1))[:10]


@pytest.mark.parametrize("k", [1, 8, 9, 128])
def test_blocks_with_their_offsets_equal_the_whole_on_the_powf_curve(k):
    """tests/test_transform_gpu.py::test_layout_bits at the new k; the cut at 253 puts every later cell into another lane group."""
    whole = _device("rand", k, 7, ab="umap")
    lo = _device("rand", k, 7, stop=253, ab="umap")
    hi = _device("rand", k, 7, first=253, query_offset=253, ab="umap")
    assert np.isfinite(whole).all() and not np.array_equal(whole, tc.layout_case("rand", k)[3])
    assert np.array_equal(_bits(np.concatenate([lo, hi])), _bits(whole))
    assert not np.array_equal(_device("rand", k, 7, first=253, query_offset=0, ab="umap"), whole[253:])
    assert np.array_equal(_bits(_device("rand", k, 7, ab="umap")), _bits(whole))
