"""ctypes binding of libgficf_harmony.so (the C ABI declared in include/gficf_harmony.h): Harmony, the batch correction of the
PCA cells.  An add-on of libgficf_hip.so, which is loaded first: it shares that library's contexts, status codes and last-error
message (``_lib.check``)."""
from __future__ import annotations

import ctypes
import os

from . import _addon, _lib

LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libgficf_harmony.so")
ABI_VERSION = 1
MAX_D, MAX_K, MAX_B, MAX_V = 128, 100, 64, 4

_i64, _i32, _int, _vp, _sz, _f64 = ctypes.c_int64, ctypes.c_int32, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double

# name -> (restype, argtypes); every symbol include/gficf_harmony.h declares
SIGNATURES = {
    "gficf_harmony_abi_version": (_int, []),
    "gficf_harmony_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64, _i64]),
    "gficf_harmony_normalise_device": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _sz]),
    "gficf_harmony_start_device": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _sz]),
    "gficf_harmony_assign_device": (_int, [_vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _f64, _vp, _vp, _vp, _vp, _sz]),
    "gficf_harmony_round_device": (_int, [_vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _f64, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _sz]),
    "gficf_harmony_objective_device": (_int, [_vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f64, _vp, _vp, _sz]),
    "gficf_harmony_correct_device": (_int, [_vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz]),
    "gficf_harmony_device": (_int, [_vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _f64, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _f64, _f64,
                                    _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz]),
    "gficf_harmony_sync": (_int, [_vp, _vp, _vp]),
}

load = _addon.loader(globals(), "gficf_harmony_abi_version")
