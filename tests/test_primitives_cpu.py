"""CPU: the probe onto the library's internal primitives (tests/helpers/prim_probe.hip) compiles for gfx950, links
libgficf_hip.so and exports its entries; the GPU tests of tests/test_primitives_gpu.py run through it."""
import ctypes
import subprocess

import pytest

from tests.helpers import prim_probe


@pytest.fixture(scope="module")
def probe_so():
    if prim_probe.hipcc() is None:
        pytest.skip("hipcc not available")
    return prim_probe.build()


def test_probe_builds_links_and_exports_its_entries(probe_so):
    L = ctypes.CDLL(probe_so)
    for name in prim_probe.SYMBOLS:
        assert hasattr(L, name), name
    dyn = subprocess.run(["nm", "-D", "--defined-only", probe_so], capture_output=True, text=True).stdout
    assert set(prim_probe.SYMBOLS) <= {ln.split()[-1] for ln in dyn.splitlines() if ln.strip()}
    need = subprocess.run(["readelf", "-d", probe_so], capture_output=True, text=True).stdout
    assert "libgficf_hip.so" in need
    # host-only entry: the count matrix of the first (widest) pass, [2^digit bits][workgroups]
    L.probe_radix_sort_hist_len.restype = ctypes.c_int64
    L.probe_radix_sort_hist_len.argtypes = [ctypes.c_int64, ctypes.c_int]
    assert L.probe_radix_sort_hist_len(1, 8) == 256
    assert L.probe_radix_sort_hist_len(4096 * 768 + 1, 32) == 256 * 768          # 4 passes of 8 bits, capped workgroups
    assert L.probe_radix_sort_hist_len(5 * 4096, 18) == 512 * 5                  # 2 passes of 9 bits
