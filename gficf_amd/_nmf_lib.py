"""ctypes binding of libgficf_nmf.so (the C ABI declared in include/gficf_nmf.h): non-negative matrix factorisation of the
GF-ICF matrix by alternating non-negative least squares.  An add-on of libgficf_hip.so, which is loaded first: it shares that
library's contexts, status codes and last-error message (``_lib.check``)."""
from __future__ import annotations

import ctypes
import os

from . import _addon, _lib

LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libgficf_nmf.so")
ABI_VERSION = 1
MAX_K = 128
NNLS_WS_BYTES = 1024

_i64, _int, _vp, _sz, _f64 = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double


def ld(k: int) -> int:
    """The row pitch of a dense operand of k columns (GFICF_NMF_LD)."""
    return (int(k) + 7) & ~7


def lp(k: int) -> int:
    """The pitch of a Gram matrix of k factors (GFICF_NMF_LP)."""
    return 16 if k <= 16 else 32 if k <= 32 else 64 if k <= 64 else 128


# name -> (restype, argtypes); every symbol include/gficf_nmf.h declares
SIGNATURES = {
    "gficf_nmf_abi_version": (_int, []),
    "gficf_nmf_workspace_bytes": (_sz, [_i64, _i64, _i64, _int]),
    "gficf_nnls_device": (_int, [_vp, _i64, _int, _vp, _int, _vp, _vp, _f64, _int, _vp, _vp, _vp, _sz]),
    "gficf_nmf_half_device": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _i64, _int, _vp, _vp, _vp, _int, _f64, _f64, _f64, _int, _vp, _vp, _vp, _vp, _vp,
                                     _sz]),
    "gficf_nmf_loss_device": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _i64, _int, _vp, _vp, _vp, _vp, _vp, _sz]),
    "gficf_nmf_device": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _i64, _int, _vp, _f64, _int, _f64, _f64, _f64, _f64, _int, _int, _vp, _vp, _vp, _vp, _vp,
                                _vp, _vp, _sz]),
    "gficf_nmf_project_device": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _i64, _int, _vp, _f64, _f64, _int, _vp, _vp, _vp, _vp, _vp, _sz]),
    "gficf_nmf_sync": (_int, [_vp, _vp]),
    "gficf_nmf_host": (_int, [_vp, _i64, _i64, _vp, _int, _vp, _vp, _int, _vp, _f64, _int, _f64, _f64, _f64, _f64, _int, _int, _vp, _vp, _vp, _vp, _vp,
                              _vp]),
    "gficf_nmf_project_host": (_int, [_vp, _i64, _i64, _vp, _int, _vp, _vp, _int, _vp, _f64, _f64, _int, _vp, _vp]),
}

load = _addon.loader(globals(), "gficf_nmf_abi_version")
