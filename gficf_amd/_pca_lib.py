"""ctypes binding of libgficf_pca.so (the C ABI declared in include/gficf_pca.h): the randomized SVD behind runPCA / runLSA /
computePCADim and the projection of new cells.  An add-on of libgficf_hip.so: it is loaded after it and shares its contexts,
status codes and last-error message (``_lib.check``)."""
from __future__ import annotations

import ctypes
import os

from . import _addon, _lib

LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libgficf_pca.so")
ABI_VERSION = 1
MAX_L = 128

_i64, _int, _vp, _sz = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t

# name -> (restype, argtypes); every symbol include/gficf_pca.h declares
SIGNATURES = {
    "gficf_pca_abi_version": (_int, []),
    "gficf_csc_tmm_workspace_bytes": (_sz, [_i64, _i64, _i64, _int]),
    "gficf_csc_tmm_device": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _int, _vp, _sz, _vp]),
    "gficf_csc_tmm_host": (_int, [_vp, _i64, _i64, _vp, _int, _vp, _vp, _vp, _int, _vp]),
    "gficf_orthonormalize_workspace_bytes": (_sz, [_i64, _int]),
    "gficf_orthonormalize_device": (_int, [_vp, _i64, _int, _vp, _vp, _sz]),
    "gficf_rsvd_workspace_bytes": (_sz, [_i64, _i64, _i64, _int]),
    "gficf_rsvd_device": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _i64, _int, _vp, _int, _int, _int, _vp, _sz, _vp, _vp, _vp, _vp]),
    "gficf_rsvd_sync": (_int, [_vp, _vp]),
    "gficf_rsvd_host": (_int, [_vp, _i64, _i64, _vp, _int, _vp, _vp, _int, _vp, _int, _int, _int, _vp, _vp, _vp, _vp]),
    "gficf_pca_project_host": (_int, [_vp, _i64, _i64, _vp, _int, _vp, _vp, _vp, _int, _vp, _vp]),
}

load = _addon.loader(globals(), "gficf_pca_abi_version")
