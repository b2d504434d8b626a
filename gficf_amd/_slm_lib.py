"""ctypes binding of libgficf_slm.so (the C ABI declared in include/gficf_slm.h): the smart local moving algorithm on the
symmetric weighted adjacency matrix of the Jaccard graph, and its sub-moving stage alone.  An add-on of libgficf_hip.so: it is
loaded after it and shares its contexts, status codes and last-error message (``_lib.check``)."""
from __future__ import annotations

import ctypes
import os

from . import _addon, _lib

LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libgficf_slm.so")
ABI_VERSION = 1

_i64, _int, _u32, _vp, _sz, _d = ctypes.c_int64, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double


class Info(ctypes.Structure):
    """gficf_slm_info"""
    _fields_ = [("n_clusters", _i64), ("start", ctypes.c_int32), ("iterations", ctypes.c_int32), ("levels", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("modularity", _d)]


class SubmoveInfo(ctypes.Structure):
    """gficf_slm_submove_info"""
    _fields_ = [("n_sub", _i64), ("passes", ctypes.c_int32), ("reserved", ctypes.c_int32)]


# name -> (restype, argtypes); every symbol include/gficf_slm.h declares
SIGNATURES = {
    "gficf_slm_abi_version": (_int, []),
    "gficf_slm_workspace_bytes": (_sz, [_i64, _i64]),
    "gficf_slm_device": (_int, [_vp, _i64, _vp, _vp, _vp, _i64, _d, _int, _int, _u32, _vp, _vp, _sz, _vp, _vp]),
    "gficf_slm_submove_device": (_int, [_vp, _i64, _vp, _vp, _vp, _i64, _d, _vp, _u32, _int, _vp, _sz, _vp, _vp]),
    "gficf_slm_host": (_int, [_vp, _i64, _vp, _vp, _vp, _i64, _d, _int, _int, _u32, _vp, _vp, _vp]),
    "gficf_slm_submove_host": (_int, [_vp, _i64, _vp, _vp, _vp, _i64, _d, _vp, _u32, _int, _vp, _vp]),
}

load = _addon.loader(globals(), "gficf_slm_abi_version")
