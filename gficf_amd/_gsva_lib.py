"""ctypes binding of libgficf_gsva.so (the C ABI declared in include/gficf_gsva.h): GSVA scores of every cell within its
cluster and the sums of the limma contrasts, the ``method="GSVA"`` branch of the reference's runGSEA().  An add-on of
libgficf_hip.so: it is loaded after it and shares its contexts, status codes and last-error message (``_lib.check``)."""
from __future__ import annotations

import ctypes
import os

from . import _addon, _lib

LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libgficf_gsva.so")
ABI_VERSION = 1
MAX_G = 131072
MAX_CELL_NZ = 4096
TILE = 256
JSPLIT = 1024

_i64, _i32, _int, _vp, _sz = ctypes.c_int64, ctypes.c_int32, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t

# name -> (restype, argtypes); every symbol include/gficf_gsva.h declares
SIGNATURES = {
    "gficf_gsva_abi_version": (_int, []),
    "gficf_gsva_workspace_bytes": (_sz, [_i64, _i64, _i32, _i64]),
    "gficf_gsva_density_device": (_int, [_vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _sz, _vp, _vp, _vp, _vp]),
    "gficf_gsva_scores_device": (_int, [_vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _i64, _i64, _i32,
                                        _vp, _sz, _vp, _vp, _vp, _vp]),
    "gficf_gsva_sync": (_int, [_vp, _vp]),
    "gficf_gsva_host": (_int, [_vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gficf_gsva_scores_host": (_int, [_vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp]),
}

load = _addon.loader(globals(), "gficf_gsva_abi_version")
