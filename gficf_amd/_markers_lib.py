"""ctypes binding of libgficf_markers.so (the C ABI declared in include/gficf_markers.h): marker genes, the one-vs-rest
Mann-Whitney U test of findClusterMarkers().  An add-on of libgficf_hip.so: it is loaded after it and shares its contexts,
status codes and last-error message (``_lib.check``)."""
from __future__ import annotations

import ctypes
import os

from . import _addon, _lib

LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libgficf_markers.so")
ABI_VERSION = 1

_i64, _int, _vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p

# name -> (restype, argtypes); every symbol include/gficf_markers.h declares
SIGNATURES = {
    "gficf_markers_abi_version": (_int, []),
    "gficf_cluster_markers_workspace_bytes": (ctypes.c_size_t, [_i64, _i64, _i64, ctypes.c_int32]),
    "gficf_cluster_markers_device": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp, ctypes.c_int32, _vp, ctypes.c_size_t, _vp, _vp]),
    "gficf_cluster_markers_sync": (_int, [_vp, _vp]),
    "gficf_cluster_markers_host": (_int, [_vp, _i64, _i64, _vp, _int, _vp, _vp, _vp, ctypes.c_int32, _vp, _vp]),
    "gficf_cluster_markers_dense_host": (_int, [_vp, _i64, _i64, _vp, _i64, _vp, _vp]),
}

load = _addon.loader(globals(), "gficf_markers_abi_version")
