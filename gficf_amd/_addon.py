"""What the ctypes bindings of the add-on libraries (``_markers_lib`` .. ``_leiden_lib``) share: their ``load()``.  A binding
module keeps its own ``LIB_PATH``, ``ABI_VERSION`` and ``SIGNATURES`` and defines ``load = _addon.loader(globals(), "<abi symbol>")``."""
from __future__ import annotations

import ctypes
import os

from . import _lib


def loader(module: dict, abi_symbol: str):
    """The memoised ``load()`` of a binding module, given its namespace (``LIB_PATH``, ``SIGNATURES`` and ``ABI_VERSION`` are
    read from it at the call, so the library is looked for where ``LIB_PATH`` points then) and the name of the symbol that
    returns the library's ABI version."""
    loaded: dict[str, ctypes.CDLL] = {}

    def load() -> ctypes.CDLL:
        path = module["LIB_PATH"]
        if path not in loaded:
            _lib.load()
            if not os.path.exists(path):
                raise ImportError(f"{path} not found: build it with `make -C gficf_amd/csrc` (hipcc, --offload-arch=gfx950)")
            L = ctypes.CDLL(path)
            for name, (res, args) in module["SIGNATURES"].items():
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
            abi = getattr(L, abi_symbol)()
            if abi != module["ABI_VERSION"]:
                raise ImportError(f"{path}: ABI {abi}, expected {module['ABI_VERSION']}")
            loaded[path] = L
        return loaded[path]

    load.__doc__ = (f"Load {os.path.basename(module['LIB_PATH'])} (after libgficf_hip.so, whose copy it then shares); raises if it "
                    "has not been built.")
    return load
