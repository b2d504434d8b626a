"""ctypes binding of libgficf_tsne.so (the C ABI declared in include/gficf_tsne.h): the perplexity graph, the exact gradient, the
layout iterations and the chained embedding behind runTsne.  An add-on of libgficf_hip.so: it is loaded after it and shares its
contexts, status codes and last-error message (``_lib.check``)."""
from __future__ import annotations

import ctypes
import os

from . import _addon, _lib

LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libgficf_tsne.so")
ABI_VERSION = 1
MAX_K = 128
TILE = 128                                   # GFICF_TSNE_TILE: the longest f32 accumulation chain of the repulsion kernel

_i64, _int, _vp, _sz, _d = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double

# name -> (restype, argtypes); every symbol include/gficf_tsne.h declares
SIGNATURES = {
    "gficf_tsne_abi_version": (_int, []),
    "gficf_tsne_affinities_workspace_bytes": (_sz, [_i64, _int]),
    "gficf_tsne_affinities_device": (_int, [_vp, _vp, _vp, _i64, _int, _i64, _d, _vp, _sz, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "gficf_tsne_shape": (_int, [_i64, _vp, _vp, _vp]),
    "gficf_tsne_gradient_device": (_int, [_vp, _i64, _vp, _vp, _vp, _i64, _vp, _d, _vp, _sz, _vp, _vp, _vp, _vp]),
    "gficf_tsne_layout_workspace_bytes": (_sz, [_i64, _i64]),
    "gficf_tsne_layout_device": (_int, [_vp, _i64, _vp, _vp, _vp, _i64, _int, _int, _int, _int, _int, _d, _d, _d, _d, _vp, _vp, _vp, _vp, _sz,
                                        _vp]),
    "gficf_tsne_sync": (_int, [_vp, _vp]),
    "gficf_tsne_host": (_int, [_vp, _vp, _i64, _int, _i64, _d, _int, _int, _int, _d, _d, _d, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}

load = _addon.loader(globals(), "gficf_tsne_abi_version")
