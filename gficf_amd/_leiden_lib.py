"""ctypes binding of libgficf_leiden.so (the C ABI declared in include/gficf_leiden.h): Leiden community detection on the
symmetric weighted adjacency matrix of the Jaccard graph, and its refinement stage alone.  An add-on of libgficf_hip.so: it is
loaded after it and shares its contexts, status codes and last-error message (``_lib.check``)."""
from __future__ import annotations

import ctypes
import os

from . import _addon, _lib

LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libgficf_leiden.so")
ABI_VERSION = 1

_i64, _int, _vp, _sz, _d = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double

# name -> (restype, argtypes); every symbol include/gficf_leiden.h declares
SIGNATURES = {
    "gficf_leiden_abi_version": (_int, []),
    "gficf_leiden_workspace_bytes": (_sz, [_i64, _i64]),
    "gficf_leiden_device": (_int, [_vp, _i64, _vp, _vp, _vp, _i64, _d, _int, _int, _vp, _vp, _vp, _vp, _vp, _sz]),
    "gficf_leiden_host": (_int, [_vp, _i64, _vp, _vp, _vp, _i64, _d, _int, _int, _vp, _vp, _vp, _vp]),
    "gficf_leiden_refine_workspace_bytes": (_sz, [_i64, _i64]),
    "gficf_leiden_refine_device": (_int, [_vp, _i64, _vp, _vp, _vp, _i64, _d, _vp, _vp, _vp, _vp, _sz]),
    "gficf_leiden_refine_host": (_int, [_vp, _i64, _vp, _vp, _vp, _i64, _d, _vp, _vp, _vp]),
}

load = _addon.loader(globals(), "gficf_leiden_abi_version")
