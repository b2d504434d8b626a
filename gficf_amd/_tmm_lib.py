"""ctypes binding of libgficf_tmm.so (the C ABI declared in include/gficf_tmm.h): edgeR's TMM library-size factors and counts
per million, the ``normalize = TRUE`` branch of the reference's gficf() and normCounts().  An add-on of libgficf_hip.so: it is
loaded after it and shares its contexts, status codes and last-error message (``_lib.check``)."""
from __future__ import annotations

import ctypes
import os

from . import _addon, _lib

LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libgficf_tmm.so")
ABI_VERSION = 1
LDS_N = 8192

_i64, _i32, _int, _vp, _sz, _f64 = ctypes.c_int64, ctypes.c_int32, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double

# name -> (restype, argtypes); every symbol include/gficf_tmm.h declares
SIGNATURES = {
    "gficf_tmm_abi_version": (_int, []),
    "gficf_tmm_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64]),
    "gficf_tmm_stats_device": (_int, [_vp, _i64, _i64, _vp, _int, _vp, _vp, _i64, _i64, _i64, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "gficf_tmm_factors_device": (_int, [_vp, _i64, _i64, _vp, _int, _vp, _vp, _i64, _i64, _i64, _vp, _f64, _f64, _i32, _i64, _i64, _i64, _i32, _vp, _sz,
                                        _vp, _vp, _vp]),
    "gficf_tmm_cpm_device": (_int, [_vp, _i64, _vp, _int, _vp, _i64, _vp, _vp, _vp, _sz, _vp]),
    "gficf_tmm_sync": (_int, [_vp, _vp]),
    "gficf_tmm_host": (_int, [_vp, _i64, _i64, _vp, _int, _vp, _vp, _i64, _f64, _f64, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                              _vp]),
}

load = _addon.loader(globals(), "gficf_tmm_abi_version")
