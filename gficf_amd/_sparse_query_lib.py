"""ctypes binding of libgficf_sparse_query.so (the C ABI declared in include/gficf_sparse_query.h): the exact kNN of new sparse
cells among the trained ones, behind ``find_nn_sparse_query``, ``umap_transform_sparse`` and ``knn_classify_sparse``.  An add-on
of libgficf_hip.so: it is loaded after it and shares its contexts, status codes and last-error message (``_lib.check``)."""
from __future__ import annotations

import ctypes
import os

from . import _addon, _lib

LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libgficf_sparse_query.so")
ABI_VERSION = 1

_i64, _int, _vp, _sz = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t

# name -> (restype, argtypes); every symbol include/gficf_sparse_query.h declares
SIGNATURES = {
    "gficf_sparse_query_abi_version": (_int, []),
    "gficf_sparse_query_shape": (_int, [_i64, _i64, _i64, _int, _vp, _vp, _vp]),
    "gficf_sparse_query_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64, _i64, _int]),
    "gficf_sparse_query_device": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _int, _int, _vp, _sz, _vp, _vp, _vp,
                                         _i64]),
    "gficf_sparse_query_sync": (_int, [_vp, _vp]),
    "gficf_sparse_query_host": (_int, [_vp, _i64, _i64, _vp, _int, _vp, _vp, _i64, _vp, _int, _vp, _vp, _int, _int, _vp, _vp]),
}

load = _addon.loader(globals(), "gficf_sparse_query_abi_version")
