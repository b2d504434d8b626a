"""ctypes binding of libgficf_umap.so (the C ABI declared in include/gficf_umap.h): the fuzzy graph, the layout sweeps and the
chained embedding behind runReduction.  An add-on of libgficf_hip.so: it is loaded after it and shares its contexts, status
codes and last-error message (``_lib.check``)."""
from __future__ import annotations

import ctypes
import os

from . import _addon, _lib

LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libgficf_umap.so")
ABI_VERSION = 1
MAX_K = 128

_i64, _int, _vp, _sz, _f, _d, _u64 = (ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_float, ctypes.c_double,
                                     ctypes.c_uint64)

# name -> (restype, argtypes); every symbol include/gficf_umap.h declares
SIGNATURES = {
    "gficf_umap_abi_version": (_int, []),
    "gficf_umap_graph_workspace_bytes": (_sz, [_i64, _int]),
    "gficf_umap_graph_device": (_int, [_vp, _vp, _vp, _i64, _int, _i64, _d, _d, _vp, _sz, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "gficf_umap_layout_workspace_bytes": (_sz, [_i64, _i64]),
    "gficf_umap_layout_device": (_int, [_vp, _i64, _vp, _vp, _vp, _i64, _f, _f, _f, _f, _int, _int, _int, _int, _u64, _vp, _vp, _sz]),
    "gficf_umap_sync": (_int, [_vp, _vp]),
    "gficf_umap_host": (_int, [_vp, _vp, _i64, _int, _i64, _int, _int, _d, _d, _d, _d, _d, _d, _int, _int, _vp, _u64, _vp, _vp, _vp, _vp, _vp,
                               _vp, _vp]),
}

load = _addon.loader(globals(), "gficf_umap_abi_version")
