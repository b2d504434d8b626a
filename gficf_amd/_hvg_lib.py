"""ctypes binding of libgficf_hvg.so (the C ABI declared in include/gficf_hvg.h): the highly variable genes of the reference's
findVarGenes(), the gene selection of ``findClusterMarkers(hvg = TRUE)``.  An add-on of libgficf_hip.so: it is loaded after it
and shares its contexts, status codes and last-error message (``_lib.check``)."""
from __future__ import annotations

import ctypes
import os

from . import _addon, _lib

LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libgficf_hvg.so")
ABI_VERSION = 1
KDE_N = 512
GRID5_MAX = 126601
GRID1_MAX = 633001
SCALARS = ("n", "k", "s0", "s1", "s2", "len5", "cdx0", "j0", "b", "a", "nls_iter", "len1", "bw", "distMid", "mu", "sigma")

_i64, _i32, _int, _vp, _sz, _f64 = ctypes.c_int64, ctypes.c_int32, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double

# name -> (restype, argtypes); every symbol include/gficf_hvg.h declares
SIGNATURES = {
    "gficf_hvg_abi_version": (_int, []),
    "gficf_hvg_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64]),
    "gficf_hvg_moments_device": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gficf_hvg_order_device": (_int, [_vp, _i64, _vp, _vp, _vp, _sz, _vp, _vp]),
    "gficf_hvg_locfit_device": (_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _sz, _vp, _vp]),
    "gficf_hvg_robust_device": (_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i32, _vp, _sz, _vp, _vp, _vp]),
    "gficf_hvg_gap_device": (_int, [_vp, _i64, _vp, _f64, _f64, _f64, _i64, _vp, _sz, _vp, _vp]),
    "gficf_hvg_curve_distance_device": (_int, [_vp, _i64, _vp, _vp, _f64, _f64, _f64, _i64, _vp, _sz, _vp, _vp]),
    "gficf_hvg_kde_device": (_int, [_vp, _i64, _vp, _vp, _sz, _vp, _vp, _vp]),
    "gficf_hvg_sync": (_int, [_vp, _vp]),
    "gficf_hvg_trend_host": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gficf_hvg_host": (_int, [_vp, _i64, _i64, _vp, _int, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}

load = _addon.loader(globals(), "gficf_hvg_abi_version")
