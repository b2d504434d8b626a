"""ctypes binding of libgficf_od.so (the C ABI declared in include/gficf_od.h): the overdispersed genes of the reference's
findOverDispersed(), the gene selection and variance scaling of ``runPCA`` / ``runLSA``.  An add-on of libgficf_hip.so that also
links libgficf_hvg.so (the gene moments): both are loaded before it, and it shares their contexts, status codes and last-error
message (``_lib.check``)."""
from __future__ import annotations

import ctypes
import os

from . import _addon, _hvg_lib, _lib

LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libgficf_od.so")
ABI_VERSION = 1
K_MAX = 8
INFO = ("n", "u", "basis", "lambda", "gcv", "edf", "vbar", "rss") + tuple(f"knot{j}" for j in range(K_MAX))

_i64, _i32, _int, _vp, _sz, _f64 = ctypes.c_int64, ctypes.c_int32, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double

# name -> (restype, argtypes); every symbol include/gficf_od.h declares
SIGNATURES = {
    "gficf_od_abi_version": (_int, []),
    "gficf_od_workspace_bytes": (_sz, [_i64, _i64]),
    "gficf_od_fit_device": (_int, [_vp, _i64, _vp, _vp, _vp, _i32, _i32, _f64, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "gficf_od_logpf_device": (_int, [_vp, _i64, _vp, _vp, _vp, _sz, _vp]),
    "gficf_od_logqchisq_device": (_int, [_vp, _i64, _vp, _f64, _vp, _sz, _vp]),
    "gficf_od_scores_device": (_int, [_vp, _i64, _vp, _vp, _vp, _i64, _f64, _f64, _vp, _sz, _vp, _vp, _vp]),
    "gficf_od_bh_log_device": (_int, [_vp, _i64, _vp, _vp, _sz, _vp]),
    "gficf_od_select_scale_device": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "gficf_od_sync": (_int, [_vp, _vp]),
    "gficf_od_from_moments_host": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _i32, _i32, _f64, _f64, _f64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gficf_od_host": (_int, [_vp, _i64, _i64, _vp, _int, _vp, _vp, _vp, _i32, _i32, _f64, _f64, _f64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                             _vp]),
    "gficf_od_select_scale_host": (_int, [_vp, _i64, _i64, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}

_load = _addon.loader(globals(), "gficf_od_abi_version")


def load() -> ctypes.CDLL:
    _hvg_lib.load()                                          # libgficf_od.so names it as a dependency: it shares the copy loaded here
    return _load()


load.__doc__ = _load.__doc__
