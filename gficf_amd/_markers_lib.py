"""ctypes binding of libgficf_markers.so (the C ABI declared in include/gficf_markers.h): marker genes, the one-vs-rest
Mann-Whitney U test of findClusterMarkers().  An add-on of libgficf_hip.so: it is loaded after it and shares its contexts,
status codes and last-error message (``_lib.check``)."""
from __future__ import annotations

import ctypes
import os

from . import _lib

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

_lib_m = None


def load() -> ctypes.CDLL:
    """Load libgficf_markers.so (after libgficf_hip.so, whose copy it then shares); raises if it has not been built."""
    global _lib_m
    if _lib_m is None:
        _lib.load()
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not found: build it with `make -C gficf_amd/csrc` (hipcc, --offload-arch=gfx950)")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.gficf_markers_abi_version() != ABI_VERSION:
            raise ImportError(f"{LIB_PATH}: ABI {L.gficf_markers_abi_version()}, expected {ABI_VERSION}")
        _lib_m = L
    return _lib_m
