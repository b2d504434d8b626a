"""ctypes binding of libgficf_gsea_exact.so (the C ABI declared in include/gficf_gsea_exact.h): the exact one-sided tail of the
enrichment score of ``gsea`` at ``gseaParam = 0``.  An add-on of libgficf_hip.so: it is loaded after it and shares its
contexts, status codes and last-error message (``_lib.check``)."""
from __future__ import annotations

import ctypes
import os

from . import _addon, _lib

LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libgficf_gsea_exact.so")
ABI_VERSION = 1
MAX_G = 131072
MAX_SIZE = 4095

_i64, _int, _vp, _sz = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t

# name -> (restype, argtypes); every symbol include/gficf_gsea_exact.h declares
SIGNATURES = {
    "gficf_gsea_exact_abi_version": (_int, []),
    "gficf_gsea_tail_workspace_bytes": (_sz, [_i64, _i64]),
    "gficf_gsea_tail_device": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _sz]),
    "gficf_gsea_tail_sync": (_int, [_vp, _vp]),
    "gficf_gsea_tail_host": (_int, [_vp, _i64, _i64, _vp, _vp, _vp]),
}

load = _addon.loader(globals(), "gficf_gsea_exact_abi_version")
