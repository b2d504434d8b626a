"""ctypes binding of libgficf_svds.so (the C ABI declared in include/gficf_svds.h): the exact truncated SVD behind
``randomized="svds"`` of runPCA / runLSA / computePCADim.  An add-on of libgficf_hip.so: it is loaded after it and shares its
contexts, status codes and last-error message (``_lib.check``)."""
from __future__ import annotations

import ctypes
import os

from . import _addon, _lib

LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libgficf_svds.so")
ABI_VERSION = 1
MAX_B = 32
MAX_M = 128

_i64, _int, _vp, _sz, _f64 = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double

# name -> (restype, argtypes); every symbol include/gficf_svds.h declares
SIGNATURES = {
    "gficf_svds_abi_version": (_int, []),
    "gficf_svds_workspace_bytes": (_sz, [_i64, _i64, _i64, _int, _int, _int]),
    "gficf_svds_device": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _i64, _int, _vp, _int, _int, _int, _f64, _int, _vp, _sz, _vp, _vp, _vp, _vp,
                                 _vp, _vp]),
    "gficf_svds_sync": (_int, [_vp, _vp]),
    "gficf_svds_host": (_int, [_vp, _i64, _i64, _vp, _int, _vp, _vp, _int, _vp, _int, _int, _int, _f64, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
}

load = _addon.loader(globals(), "gficf_svds_abi_version")
