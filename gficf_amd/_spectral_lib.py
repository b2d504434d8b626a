"""ctypes binding of libgficf_spectral.so (the C ABI declared in include/gficf_spectral.h): the connected components of a CSR
graph and the leading eigenvectors of its normalised Laplacian, the spectral start of the embedding.  An add-on of
libgficf_hip.so: it is loaded after it and shares its contexts, status codes and last-error message (``_lib.check``)."""
from __future__ import annotations

import ctypes
import os

from . import _addon, _lib

LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libgficf_spectral.so")
ABI_VERSION = 1
MAX_NDIM = 8
MAX_M = 64

_i64, _int, _vp, _sz, _d = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double

# name -> (restype, argtypes); every symbol include/gficf_spectral.h declares
SIGNATURES = {
    "gficf_spectral_abi_version": (_int, []),
    "gficf_graph_components_workspace_bytes": (_sz, [_i64]),
    "gficf_graph_components_device": (_int, [_vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _sz]),
    "gficf_spectral_workspace_bytes": (_sz, [_i64, _i64, _int, _int]),
    "gficf_spectral_device": (_int, [_vp, _i64, _vp, _vp, _vp, _i64, _int, _vp, _d, _int, _int, _vp, _sz, _vp, _vp, _vp, _vp]),
    "gficf_spectral_host": (_int, [_vp, _i64, _vp, _vp, _vp, _int, _vp, _d, _int, _int, _vp, _vp, _vp, _vp, _vp]),
}

load = _addon.loader(globals(), "gficf_spectral_abi_version")
