"""ctypes binding of libgficf_transform.so (the C ABI declared in include/gficf_transform.h): the rectangular search, the
memberships, the initial positions, the one-launch layout and the vote behind embedNewCells / classify_cells.  An add-on of
libgficf_hip.so: it is loaded after it and shares its contexts, status codes and last-error message (``_lib.check``)."""
from __future__ import annotations

import ctypes
import os

from . import _addon, _lib

LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libgficf_transform.so")
ABI_VERSION = 1
MAX_K = 128

_i64, _int, _vp, _sz, _f, _d, _u64 = (ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_float, ctypes.c_double,
                                     ctypes.c_uint64)

# name -> (restype, argtypes); every symbol include/gficf_transform.h declares
SIGNATURES = {
    "gficf_transform_abi_version": (_int, []),
    "gficf_transform_search_split": (_int, [_vp, _i64, _i64]),
    "gficf_transform_search_workspace_bytes": (_sz, [_i64, _i64, _int]),
    "gficf_transform_search_device": (_int, [_vp, _vp, _i64, _vp, _i64, _int, _int, _int, _vp, _sz, _vp, _vp, _i64]),
    "gficf_transform_weights_workspace_bytes": (_sz, [_i64, _int]),
    "gficf_transform_weights_device": (_int, [_vp, _vp, _vp, _i64, _i64, _int, _i64, _d, _vp, _sz, _vp, _i64, _vp, _vp]),
    "gficf_transform_init_workspace_bytes": (_sz, [_i64, _int]),
    "gficf_transform_init_device": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _int, _vp, _sz, _vp]),
    "gficf_transform_layout_workspace_bytes": (_sz, [_i64, _int]),
    "gficf_transform_layout_device": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _int, _f, _f, _f, _f, _int, _int, _int, _int, _u64, _i64,
                                             _vp, _vp, _sz]),
    "gficf_transform_vote_workspace_bytes": (_sz, [_i64, _int]),
    "gficf_transform_vote_device": (_int, [_vp, _vp, _i64, _vp, _i64, _i64, _int, _int, _vp, _sz, _vp, _vp]),
    "gficf_transform_sync": (_int, [_vp, _vp]),
    "gficf_transform_search_host": (_int, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _int, _int, _int, _vp, _vp]),
    "gficf_transform_host": (_int, [_vp, _vp, _i64, _i64, _vp, _vp, _i64, _i64, _int, _int, _int, _d, _d, _d, _d, _d, _int, _int, _int, _int, _vp,
                                    _u64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gficf_transform_classify_host": (_int, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _int, _int, _int, _vp, _int, _vp]),
}

load = _addon.loader(globals(), "gficf_transform_abi_version")
