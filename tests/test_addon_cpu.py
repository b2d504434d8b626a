"""No GPU: what the add-on libraries share (gficf_amd/_addon.py, csrc/addon_status.h, csrc/knn_symmetrise.h) seen from outside.
The workspace sizes are host queries, so the byte layout the shared carve must keep is checked here against the values the
libraries gave before they shared it; the loaders are checked for what every binding module promised on its own before."""
import ctypes
import importlib
import os

import pytest

from gficf_amd import _spectral_lib, _transform_lib, _tsne_lib, _umap_lib

ADDONS = ("markers", "pca", "umap", "transform", "gsea", "tsne", "spectral", "leiden")

SHAPES = [(N, k) for N in (1, 2, 255, 256, 257, 54000) for k in (2, 15, 128)]
TRAIN = 54000                                                       # training rows of the transform's search, M = N queries


def workspace_bytes(N: int, k: int) -> tuple:
    """Every workspace query of the graph add-ons for N points and k columns, at the capacities that go with them."""
    um, ts, tr, sp = _umap_lib.load(), _tsne_lib.load(), _transform_lib.load(), _spectral_lib.load()
    return (
        um.gficf_umap_graph_workspace_bytes(N, k),
        um.gficf_umap_layout_workspace_bytes(N, 2 * N * k),
        um.gficf_umap_layout_workspace_bytes(N, 0),
        ts.gficf_tsne_affinities_workspace_bytes(N, k),
        ts.gficf_tsne_layout_workspace_bytes(N, 2 * N * (k - 1)),
        tr.gficf_transform_search_workspace_bytes(N, TRAIN, k),
        tr.gficf_transform_search_workspace_bytes(257, N, k),
        tr.gficf_transform_weights_workspace_bytes(N, k),
        tr.gficf_transform_init_workspace_bytes(N, k),
        tr.gficf_transform_layout_workspace_bytes(N, k),
        tr.gficf_transform_vote_workspace_bytes(N, k),
        sp.gficf_spectral_workspace_bytes(N, 2 * N * k, 2, 32),
        sp.gficf_graph_components_workspace_bytes(N),
    )


# (N, k) -> workspace_bytes(N, k), printed by `python -m tests.test_addon_cpu` on the commit before the add-ons shared their
# symmetrisation (libraries built with `make -C gficf_amd/csrc`)
RECORDED = {
    (1, 2): (4096, 2304, 2304, 2816, 2304, 4096, 4864, 512, 512, 512, 512, 104448, 1024),
    (1, 15): (4096, 2304, 2304, 2816, 2304, 25856, 31488, 512, 512, 512, 512, 104448, 1024),
    (1, 128): (13056, 3072, 2304, 11520, 2304, 216576, 263680, 512, 512, 512, 512, 104448, 1024),
    (2, 2): (4096, 2304, 2304, 2816, 2304, 7424, 4864, 512, 512, 512, 512, 104960, 1024),
    (2, 15): (4864, 2304, 2304, 3584, 2304, 51200, 31488, 512, 512, 512, 512, 104960, 1024),
    (2, 128): (23808, 4096, 2304, 22272, 2304, 432640, 263680, 512, 512, 512, 512, 104960, 1024),
    (255, 2): (46848, 7936, 4096, 24064, 13824, 522752, 4864, 512, 512, 512, 512, 254208, 1024),
    (255, 15): (328448, 34560, 4096, 305664, 13824, 3917312, 31488, 512, 512, 512, 512, 254208, 1024),
    (255, 128): (2776576, 265728, 4096, 2755584, 13824, 33423872, 263680, 512, 512, 512, 512, 254976, 1024),
    (256, 2): (49152, 7936, 4096, 26368, 13824, 524800, 4864, 512, 512, 512, 512, 254720, 1024),
    (256, 15): (332800, 34560, 4096, 310016, 13824, 3932672, 31488, 512, 512, 512, 512, 254720, 1024),
    (256, 128): (2820096, 267008, 4096, 2797312, 13824, 33554944, 263680, 512, 512, 512, 512, 255744, 1024),
    (257, 2): (50944, 8448, 4352, 28160, 18688, 424192, 4864, 512, 512, 512, 512, 257024, 1024),
    (257, 15): (334592, 35072, 4352, 311808, 18688, 3177216, 31488, 512, 512, 512, 512, 257024, 1024),
    (257, 128): (2834944, 268288, 4352, 2807808, 18688, 27106816, 263680, 512, 512, 512, 512, 258048, 1024),
    (54000, 2): (9182720, 1301248, 434176, 4592640, 9554432, 864512, 424192, 512, 512, 512, 512, 32289792, 1024),
    (54000, 15): (68853760, 6939136, 434176, 64262656, 9554432, 6480640, 3177216, 512, 512, 512, 512, 32311552, 1024),
    (54000, 128): (582182912, 55945728, 434176, 577646336, 9554432, 55296512, 27106816, 512, 512, 512, 512, 32502272, 1024),
}


@pytest.mark.parametrize("N,k", SHAPES)
def test_workspace_bytes_are_the_recorded_ones(N, k):
    assert workspace_bytes(N, k) == RECORDED[(N, k)]


@pytest.mark.parametrize("name", ADDONS)
def test_loader(name, monkeypatch):
    mod = importlib.import_module(f"gficf_amd._{name}_lib")
    L = mod.load()
    assert isinstance(L, ctypes.CDLL) and mod.load() is L
    abi = [s for s in mod.SIGNATURES if s.endswith("_abi_version")]
    assert len(abi) == 1 and getattr(L, abi[0])() == mod.ABI_VERSION
    for sym, (res, args) in mod.SIGNATURES.items():
        fn = getattr(L, sym)
        assert fn.restype is res and list(fn.argtypes) == list(args), sym
    assert os.path.basename(mod.LIB_PATH) == f"libgficf_{name}.so"
    monkeypatch.setattr(mod, "LIB_PATH", os.path.join(os.path.dirname(mod.LIB_PATH), f"libgficf_{name}_missing.so"))
    with pytest.raises(ImportError, match="not found: build it with"):
        mod.load()
    monkeypatch.undo()
    assert mod.load() is L


def test_loader_refuses_another_abi(monkeypatch):
    monkeypatch.setattr(_umap_lib, "ABI_VERSION", _umap_lib.ABI_VERSION + 1)
    # the same file under a name that has not been loaded yet: load() remembers a library by its path
    monkeypatch.setattr(_umap_lib, "LIB_PATH", os.path.join(os.path.dirname(_umap_lib.LIB_PATH), ".", "libgficf_umap.so"))
    with pytest.raises(ImportError, match=r"ABI 1, expected 2"):
        _umap_lib.load()


if __name__ == "__main__":
    for shape in SHAPES:
        print(f"    {shape}: {workspace_bytes(*shape)},")
