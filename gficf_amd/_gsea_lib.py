"""ctypes binding of libgficf_gsea.so (the C ABI declared in include/gficf_gsea.h): gene-set enrichment of every cluster's
gene ranking, the fgsea call inside runGSEA().  An add-on of libgficf_hip.so: it is loaded after it and shares its contexts,
status codes and last-error message (``_lib.check``)."""
from __future__ import annotations

import ctypes
import os

from . import _addon, _lib

LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libgficf_gsea.so")
ABI_VERSION = 1
MAX_G = 131072

_i64, _i32, _u32, _int, _vp, _sz = ctypes.c_int64, ctypes.c_int32, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t

# name -> (restype, argtypes); every symbol include/gficf_gsea.h declares
SIGNATURES = {
    "gficf_gsea_abi_version": (_int, []),
    "gficf_gsea_perm_batch": (_i64, [_i64, _i64]),
    "gficf_gsea_workspace_bytes": (_sz, [_i64, _i32, _i64, _i64, _i32, _i64]),
    "gficf_gsea_device": (_int, [_vp, _i64, _i32, _vp, _i64, _vp, _vp, _i64, _i32, _vp, _vp, _i64, _u32, _vp, _sz, _vp, _vp, _vp, _vp]),
    "gficf_gsea_sync": (_int, [_vp, _vp]),
    "gficf_gsea_host": (_int, [_vp, _i64, _i32, _vp, _i64, _vp, _vp, _i64, _u32, _i64, _i64, _vp, _vp, _vp, _vp, _i64]),
    "gficf_gsea_permutation_host": (_int, [_vp, _i64, _u32, _i64, _vp]),
}

load = _addon.loader(globals(), "gficf_gsea_abi_version")
