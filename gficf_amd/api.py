"""Host-side mirror of the reference's operator interface for the hot path.

Two layers over the C ABI (include/gficf_hip.h):

* reference-shaped functions on host data, same names / argument meaning / error
  behaviour as the R package, so that parity tests read like the reference's own calls:
    - ``rcpp_parallel_jaccard_coef(mat, printOutput)``   reference R/RcppExports.R:16-18
    - ``jaccard_coeff(idx, printOutput)``                reference R/RcppExports.R:8-10 (the serial entry)
    - ``jaccard_edges(neigh, verbose)``                  reference R/clustCells.R:63-68
    - ``gficf(M, cell_proportion_max, cell_proportion_min, storeRaw, normalize, verbose)``
                                                         reference R/gficf.R:17-33
    - ``gficf_with_weights(M, w)``                       reference R/cellClassifier.R:50-53
    - ``runPCA`` / ``runLSA`` / ``computePCADim``        reference R/dimensinalityReduction.R:19-133,206-230 (libgficf_pca.so)
    - ``runReduction(data, reduction, ...)``             reference R/dimensinalityReduction.R:157-192 (libgficf_umap.so)
* ``HipOps``: the device-resident pipeline stages on torch CUDA tensors (torch is only
  the owner of device memory / streams here), used by the bench and the multi-GPU path.

All compute happens in libgficf_hip.so; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import warnings

import numpy as np

from . import _lib
from ._lib import GficfError, check


# ---------------------------------------------------------------------------- context
class Context:
    """One libgficf_hip context (device + stream + workspace)."""

    def __init__(self, device: int = 0, stream: int | None = None):
        self._h = ctypes.c_void_p()
        check(_lib.load().gficf_ctx_create(int(device), ctypes.c_void_p(stream or 0), ctypes.byref(self._h)))
        self.device = int(device)
        self._stream = int(stream or 0)          # what the library's context is bound to (set_stream skips the call when unchanged)

    @property
    def handle(self):
        if not self._h:
            raise RuntimeError("context is closed")
        return self._h

    def set_stream(self, stream: int | None):
        s = int(stream or 0)
        if s != self._stream:
            check(_lib.load().gficf_ctx_set_stream(self.handle, ctypes.c_void_p(s)))
            self._stream = s

    def sync(self):
        """Wait for the stream; raises GficfError for deferred input-validation failures."""
        check(_lib.load().gficf_ctx_sync(self.handle))

    def set_jaccard_distinct(self, assume_distinct: bool):
        """Rows of the kNN index matrix are taken to hold distinct ids (what every kNN search returns): the ingest skips its
        all-pairs duplicate scan and the edge kernel raises a deferred ``GFICF_ERR_DUPLICATE_IDS`` at the next :meth:`sync` if
        a row does repeat an id — discard the edges then and re-run ingest + edges with the option off.  Only for the
        single-context sequence over all cells (``gficf_ctx_set_jaccard_distinct``); the host entries do this by themselves."""
        check(_lib.load().gficf_ctx_set_jaccard_distinct(self.handle, 1 if assume_distinct else 0))

    def set_jaccard_direct_max_edges(self, max_edges: int):
        """Edges (N * k) up to which the single-device Jaccard sequence runs as ONE launch without a table, k <= 32, rows taken
        to hold distinct ids (``gficf_ctx_set_jaccard_direct_max_edges``); -1 = the build's default, 0 = never."""
        check(_lib.load().gficf_ctx_set_jaccard_direct_max_edges(self.handle, int(max_edges)))

    def close(self):
        if self._h:
            _lib.load().gficf_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx: dict[int, Context] = {}


def default_context(device: int = 0) -> Context:
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


def device_count() -> int:
    n = ctypes.c_int(0)
    rc = _lib.load().gficf_device_count(ctypes.byref(n))
    return n.value if rc == 0 else 0


def _np_ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class MultiContext:
    """Several GPUs of one node behind the host entry points, single process (``gficf_multi_*`` of the C ABI): cells
    shard by contiguous block, one context and one stream per device.  ``devices``: HIP ordinals; the same ordinal may be
    named more than once (one block each)."""

    def __init__(self, devices):
        devices = [int(d) for d in devices]
        if not devices:
            raise ValueError("devices must name at least one GPU")
        arr = (ctypes.c_int * len(devices))(*devices)
        self._h = ctypes.c_void_p()
        check(_lib.load().gficf_multi_create(arr, len(devices), ctypes.byref(self._h)))
        self.devices = devices

    @property
    def handle(self):
        if not self._h:
            raise RuntimeError("multi context is closed")
        return self._h

    # ---- the device-resident step: blocks already in HBM, table slices exchanged by direct peer copies
    def cell_blocks(self, N: int) -> list[int]:
        """bounds[r] .. bounds[r + 1] = cells of device slot r (``gficf_multi_cell_blocks``)."""
        bd = (ctypes.c_int64 * (len(self.devices) + 1))()
        check(_lib.load().gficf_multi_cell_blocks(int(N), len(self.devices), bd))
        return list(bd)

    def set_jaccard_distinct(self, assume_distinct: bool):
        check(_lib.load().gficf_multi_set_jaccard_distinct(self.handle, 1 if assume_distinct else 0))

    def jaccard_device(self, idx_blocks, N: int, k: int, tables, outs):
        """``gficf_multi_jaccard_device``: ``idx_blocks[r]`` the (k, n_r) int32 / float64 tensor of block r on device slot r
        (column-major n_r x k, global 1-based ids), ``tables[r]`` an (N, row_words) int32 tensor and ``outs[r]`` a (3, n_r*k)
        float64 tensor on the same device.  Enqueues only (on the contexts' own streams: the inputs must be complete —
        synchronise the torch streams that made them first); :meth:`sync` waits and raises deferred errors."""
        P = len(self.devices)
        if not (len(idx_blocks) == len(tables) == len(outs) == P):
            raise ValueError("one block, table and output per device slot")
        bd = self.cell_blocks(N)
        f64 = {str(t.dtype) for t in idx_blocks if t is not None and t.numel()}
        if len(f64) > 1 or (f64 and f64 - {"torch.int32", "torch.float64"}):
            raise ValueError("idx blocks must all be int32 or all float64")
        is_f64 = 1 if f64 == {"torch.float64"} else 0
        ptr = lambda ts: (ctypes.c_void_p * P)(*[(t.data_ptr() if t is not None and t.numel() else None) for t in ts])
        lds = (ctypes.c_int64 * P)(*[(int(t.shape[1]) if t is not None and t.dim() == 2 else bd[r + 1] - bd[r]) for r, t in enumerate(idx_blocks)])
        for r in range(P):
            n = bd[r + 1] - bd[r]
            if n > 0 and (tuple(outs[r].shape) != (3, n * k) or str(outs[r].dtype) != "torch.float64" or not outs[r].is_contiguous()):
                raise ValueError(f"outs[{r}] must be a contiguous float64 tensor of shape (3, {n * k})")
            if not tables[r].is_contiguous() or (n > 0 and not idx_blocks[r].is_contiguous()):
                raise ValueError("expected contiguous tensors")
        check(_lib.load().gficf_multi_jaccard_device(self.handle, ptr(idx_blocks), is_f64, lds, int(N), int(k), ptr(tables), ptr(outs)))

    def halo_buffers(self, N: int, k: int, cap: int | None = None) -> dict:
        """Per-device buffers of :meth:`jaccard_halo_device` (allocated once, reused by every step): the plan's workspace (zeroed
        here, once), request slots, the sub-problem's table and local -> global map, the block's output."""
        import torch

        L = _lib.load()
        P = len(self.devices)
        bd = self.cell_blocks(N)
        rpr = -(-max(int(N), 1) // P)
        if cap is None:
            room = (1 << 17) - 1 - rpr                                   # rows left below 2^17 next to the largest block (compact rows)
            cap = max(64, min(8192, room // P)) if room >= 64 * P else 1024
        wsb = int(L.gficf_jaccard_halo_workspace_bytes(int(N), P))
        bufs = dict(cap=int(cap), ws=[], req=[], table=[], l2g=[], out=[])
        for r, d in enumerate(self.devices):
            n = bd[r + 1] - bd[r]
            n_ext = n + P * cap
            dev = torch.device("cuda", d)
            roww = int(L.gficf_jaccard_row_words(n_ext, int(k)))
            if roww < 0:
                raise GficfError(5, f"k = {k} / {n_ext} rows: no table format")
            bufs["ws"].append(torch.zeros(wsb, dtype=torch.uint8, device=dev))
            bufs["req"].append(torch.zeros(P * cap, dtype=torch.int32, device=dev))
            bufs["table"].append(torch.zeros((n_ext, roww), dtype=torch.int32, device=dev))
            bufs["l2g"].append(torch.zeros(n_ext, dtype=torch.int32, device=dev))
            bufs["out"].append(torch.zeros((3, n * k), dtype=torch.float64, device=dev))
        return bufs

    def jaccard_halo_device(self, idx_blocks, N: int, k: int, bufs: dict):
        """``gficf_multi_jaccard_halo_device``: the device-resident step for blocks whose ids have locality — nothing is exchanged,
        a device reads the few rows its block names outside where they lie, in the other devices' blocks (peer mapping).  ``idx_blocks[r]``:
        the (k, n_r) int32 tensor of block r on device slot r; ``bufs`` from :meth:`halo_buffers` (results in ``bufs["out"][r]``).
        The step is POSTED to per-device host threads and the call returns before anything is enqueued: the inputs must be complete
        before the call (synchronise the torch streams that produced them) and :meth:`sync` is the ONLY completion point — the blocks
        of ids and ``bufs`` must stay unchanged until it has returned (an event recorded after this call orders nothing).  ``sync``
        also raises the deferred errors (``GFICF_ERR_CAPACITY``: ids without locality).  ``bufs["ws"]`` must be all-zero at the
        first step (:meth:`halo_buffers` allocates it so; the library keeps it consistent afterwards)."""
        P = len(self.devices)
        if len(idx_blocks) != P:
            raise ValueError("one block per device slot")
        bd = self.cell_blocks(N)
        for r, t in enumerate(idx_blocks):
            if bd[r + 1] - bd[r] > 0 and (str(t.dtype) != "torch.int32" or not t.is_contiguous() or t.dim() != 2 or t.shape[0] != k):
                raise ValueError(f"idx_blocks[{r}] must be a contiguous int32 tensor of shape ({k}, n_r)")
        ptr = lambda ts: (ctypes.c_void_p * P)(*[(t.data_ptr() if t is not None and t.numel() else None) for t in ts])
        lds = (ctypes.c_int64 * P)(*[(int(t.shape[1]) if t is not None and t.dim() == 2 and t.numel() else bd[r + 1] - bd[r]) for r, t in enumerate(idx_blocks)])
        check(_lib.load().gficf_multi_jaccard_halo_device(self.handle, ptr(idx_blocks), lds, int(N), int(k), int(bufs["cap"]), ptr(bufs["ws"]), ptr(bufs["req"]),
                                                          ptr(bufs["table"]), ptr(bufs["l2g"]), ptr(bufs["out"])))

    def sync(self):
        check(_lib.load().gficf_multi_sync(self.handle))

    def close(self):
        if self._h:
            _lib.load().gficf_multi_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_multi_ctx: dict[tuple, MultiContext] = {}


def env_devices():
    """The device list of the environment variable GFICF_HIP_DEVICES ("0,1,2,3"), which is what the R glue reads; None when
    it is unset or names a single device."""
    import os

    e = os.environ.get("GFICF_HIP_DEVICES", "").strip()
    if not e:
        return None
    devs = [int(t) for t in e.replace(";", ",").split(",") if t.strip() != ""]
    return devs if len(devs) > 1 else None


def _multi(devices) -> MultiContext | None:
    if devices is None:
        devices = env_devices()
    if devices is None:
        return None
    key = tuple(int(d) for d in devices)
    if key not in _multi_ctx:
        _multi_ctx[key] = MultiContext(key)
    return _multi_ctx[key]


def _knn_matrix(mat, name="mat"):
    """The kNN index matrix as the C ABI takes it: Fortran-ordered int32 (integer input) or float64 (anything else, what
    Rcpp coerces to).  Integer ids that do not fit int32 cannot be valid (N <= 2^31 - 1): rejected here, before the
    narrowing cast could alias them onto valid ids."""
    mat = np.asarray(mat)
    if mat.ndim != 2:
        raise ValueError(f"{name} must be a 2-d matrix")
    if np.issubdtype(mat.dtype, np.integer):
        if mat.dtype != np.int32 and mat.size and (int(mat.min()) < -2 ** 31 or int(mat.max()) > 2 ** 31 - 1):
            raise GficfError(2, "kNN index matrix holds an id outside [1, N] or a non-integer value")
        return np.asfortranarray(mat, dtype=np.int32), 0
    return np.asfortranarray(mat, dtype=np.float64), 1


# ------------------------------------------------------------- Jaccard, reference-shaped
def rcpp_parallel_jaccard_coef(mat, printOutput: bool = False, ctx: Context | None = None, devices=None,
                               truncate_noninteger_ids: bool = False) -> np.ndarray:
    """Drop-in for the reference's ``rcpp_parallel_jaccard_coef(mat, printOutput)``.

    ``mat``: N x k matrix of 1-based neighbour ids (integer or float64, as R hands it over:
    reference R/clustCells.R:63-65).  Returns the (N*k) x 3 float64 matrix (Fortran order,
    like an R matrix) whose row i*k+j is (i+1, mat[i,j], u/(2k-u)) or zeros when the two
    neighbour sets do not intersect (reference src/rcpp_parallel_jaccard_coeff.cpp:48-52,67).

    ``devices`` (or the environment variable GFICF_HIP_DEVICES): a list of GPUs to shard the cells over, single process
    (``gficf_jaccard_host_multi``); same result.

    ``truncate_noninteger_ids``: strict drop-in mode for ids given as non-integer doubles (rejected by default): the
    reference's ``int k = mat(i,j) - 1`` (src/rcpp_parallel_jaccard_coeff.cpp:28) — the row is addressed by truncation, the
    rows are intersected as the doubles they hold (``gficf_ctx_set_jaccard_options``; single device).
    """
    m, is_f64 = _knn_matrix(mat)
    N, k = m.shape
    E = N * k
    rm = np.zeros((3, E), dtype=np.float64)  # C-order (3, E) == column-major (E, 3)
    if truncate_noninteger_ids:
        ctx = ctx or default_context()
        L = _lib.load()
        check(L.gficf_ctx_set_jaccard_options(ctx.handle, 1))
        try:
            check(L.gficf_jaccard_host(ctx.handle, _np_ptr(m), is_f64, N, k, max(N, 1), _np_ptr(rm), 1 if printOutput else 0))
        finally:
            L.gficf_ctx_set_jaccard_options(ctx.handle, 0)
        return rm.T
    mc = _multi(devices) if ctx is None else None
    if mc is not None:
        check(_lib.load().gficf_jaccard_host_multi(mc.handle, _np_ptr(m), is_f64, N, k, max(N, 1), _np_ptr(rm),
                                                   1 if printOutput else 0))
        return rm.T
    ctx = ctx or default_context()
    check(_lib.load().gficf_jaccard_host(ctx.handle, _np_ptr(m), is_f64, N, k, max(N, 1), _np_ptr(rm),
                                         1 if printOutput else 0))
    return rm.T


def jaccard_counts(mat, ctx: Context | None = None) -> np.ndarray:
    """The intersection counts u[i, j] = |row i ∩ row mat[i, j]| alone (uint16, N x k): the compact return of the C ABI
    (``gficf_jaccard_counts_host``, 2 B per edge across PCIe instead of the reference's 24 B row)."""
    m, is_f64 = _knn_matrix(mat)
    N, k = m.shape
    u = np.zeros((N, k), dtype=np.uint16)
    ctx = ctx or default_context()
    check(_lib.load().gficf_jaccard_counts_host(ctx.handle, _np_ptr(m), is_f64, N, k, max(N, 1), _np_ptr(u)))
    return u


def jaccard_expand(mat, u, n_threads: int = 0) -> np.ndarray:
    """Counts -> the reference's (N*k) x 3 edge matrix, on the host (``gficf_jaccard_expand_host``; no device)."""
    m, is_f64 = _knn_matrix(mat)
    N, k = m.shape
    u = np.ascontiguousarray(u, dtype=np.uint16)
    if u.shape != (N, k):
        raise ValueError("u must have the shape of mat")
    rm = np.zeros((3, N * k), dtype=np.float64)
    check(_lib.load().gficf_jaccard_expand_host(_np_ptr(m), is_f64, N, k, max(N, 1), _np_ptr(u), _np_ptr(rm), int(n_threads)))
    return rm.T


def jaccard_coeff(idx, printOutput: bool = False, ctx: Context | None = None) -> np.ndarray:
    """Drop-in for the reference's serial ``jaccard_coeff(idx, printOutput)`` (reference R/RcppExports.R:8-10,
    src/jaccard_coeff.cpp:19-44): the same edges as :func:`rcpp_parallel_jaccard_coef`, but the rows with u > 0 follow
    one another from the top of the (N*k) x 3 matrix (the rest is zero) and the intersection is of the rows as sets
    (``Rcpp::intersect``; only rows that hold an id twice can tell)."""
    m, is_f64 = _knn_matrix(idx, "idx")
    N, k = m.shape
    w = np.zeros((3, N * k), dtype=np.float64)      # C-order (3, E) == column-major (E, 3)
    ctx = ctx or default_context()
    check(_lib.load().gficf_jaccard_coeff_host(ctx.handle, _np_ptr(m), is_f64, N, k, max(N, 1), _np_ptr(w), 1 if printOutput else 0))
    return w.T


def jaccard_edges(neigh, verbose: bool = False, ctx: Context | None = None):
    """The Jaccard call-site of ``clustcells()`` (reference R/clustCells.R:63-68).

    ``neigh``: N x (k+1) kNN index matrix whose first column is the cell itself
    (``uwot:::find_nn(..., include_self = TRUE)$idx``).  Drops column 1, builds the Jaccard
    edges and keeps the rows with weight > 0, in order.  Returns a dict with float64
    arrays ``from``, ``to``, ``weight`` (the columns of the reference's data.frame).
    """
    neigh = np.asarray(neigh)[:, 1:]                                   # :63
    if verbose:
        print("Running Parallell Jaccard Coefficient Estimation...")
    m, is_f64 = _knn_matrix(neigh, "neigh")
    N, k = m.shape
    ctx = ctx or default_context()
    L = _lib.load()
    n = ctypes.c_int64(0)
    # :65 and the weight > 0 filter of :66 in one device pass; only the kept edges cross PCIe
    check(L.gficf_jaccard_filtered_host_plan(ctx.handle, _np_ptr(m), is_f64, N, k, max(N, 1), ctypes.byref(n)))
    out = {key: np.empty(n.value, dtype=np.float64) for key in ("from", "to", "weight")}                  # :67-68
    check(L.gficf_jaccard_filtered_host_finish(ctx.handle, _np_ptr(out["from"]), _np_ptr(out["to"]), _np_ptr(out["weight"])))
    if verbose:
        print("Done!!")
    return out


def jaccard_adjacency(edges: dict, N: int, ctx: Context | None = None):
    """The kept edges as the symmetric weighted adjacency matrix of the undirected graph —
    ``igraph::as_adjacency_matrix(igraph::graph.data.frame(relations, directed = FALSE), attr = "weight", sparse = T)``
    (reference R/clustCells.R:69,80,86), the input of the modularity optimiser.  ``edges``: the dict of
    :func:`jaccard_edges` (``from`` / ``to`` / ``weight``); ``N``: number of cells.  Returns a scipy CSC matrix
    (N x N, sorted indices): A[i,j] = A[j,i] = sum of the weights of the edges between i and j."""
    import scipy.sparse as sp

    f = np.ascontiguousarray(edges["from"], dtype=np.float64)
    t = np.ascontiguousarray(edges["to"], dtype=np.float64)
    w = np.ascontiguousarray(edges["weight"], dtype=np.float64)
    if not (f.shape == t.shape == w.shape and f.ndim == 1):
        raise ValueError("from / to / weight must be 1-d arrays of the same length")
    ctx = ctx or default_context()
    L = _lib.load()
    nnz = ctypes.c_int64(0)
    check(L.gficf_adjacency_host_plan(ctx.handle, int(N), len(f), _np_ptr(f), _np_ptr(t), _np_ptr(w), ctypes.byref(nnz)))
    indptr = np.zeros(N + 1, dtype=np.int64)
    indices = np.zeros(nnz.value, dtype=np.int32)
    x = np.zeros(nnz.value, dtype=np.float64)
    check(L.gficf_adjacency_host_finish(ctx.handle, _np_ptr(indptr), 1, _np_ptr(indices), _np_ptr(x)))
    return sp.csc_matrix((x, indices, indptr), shape=(N, N))


# -------------------------------------------------------------- GF-ICF, reference-shaped
def _csc_parts(M):
    import scipy.sparse as sp

    if not sp.isspmatrix_csc(M):
        M = sp.csc_matrix(M)
    if not M.has_sorted_indices:
        M = M.copy()
        M.sort_indices()
    colptr = np.ascontiguousarray(M.indptr)
    if colptr.dtype not in (np.int32, np.int64):
        colptr = colptr.astype(np.int64)
    rowidx = np.ascontiguousarray(M.indices, dtype=np.int32)
    x = np.ascontiguousarray(M.data, dtype=np.float64)
    return M, colptr, rowidx, x


ICF_TYPES = {"classic": 0, "prob": 1, "smooth": 2}      # getIdfW(type = ...), reference R/gficf.R:89-91
NORMS = {"l2": 0, "l1": 1}                               # l.norm(norm = ...), reference R/gficf.R:100


def _normalize_csc_host(M, prop_min, prop_max, w_in, ctx, icf_type="classic", norm="l2", devices=None, raw=False):
    import scipy.sparse as sp

    if icf_type not in ICF_TYPES or norm not in NORMS:
        raise ValueError("icf_type must be classic / prob / smooth and norm l2 / l1")
    M, colptr, rowidx, x = _csc_parts(M)
    G, N = M.shape
    L = _lib.load()
    mc = _multi(devices) if ctx is None else None
    if mc is not None and (icf_type != "classic" or norm != "l2"):
        # the multi-GPU entry runs gficf() as the reference calls it (icf_type classic, norm l2).  A device list passed
        # by the caller together with other options is a contradiction; one that only came from GFICF_HIP_DEVICES must
        # not break a call that works without the variable: the helper branches run on the default device.
        if devices is not None:
            raise ValueError("the multi-GPU entry runs gficf() as the reference calls it: icf_type classic, norm l2")
        mc = None
    if mc is not None:
        return _normalize_csc_host_run(L, mc, M, colptr, rowidx, x, G, N, prop_min, prop_max, w_in,
                                       L.gficf_normalize_csc_host_multi_plan, L.gficf_normalize_csc_host_multi_finish, raw=raw)
    ctx = ctx or default_context()
    check(L.gficf_ctx_set_gficf_options(ctx.handle, ICF_TYPES[icf_type], NORMS[norm]))
    try:
        return _normalize_csc_host_run(L, ctx, M, colptr, rowidx, x, G, N, prop_min, prop_max, w_in, raw=raw)
    finally:
        L.gficf_ctx_set_gficf_options(ctx.handle, 0, 0)


def _normalize_csc_host_run(L, ctx, M, colptr, rowidx, x, G, N, prop_min, prop_max, w_in, plan=None, finish=None, raw=False):
    """plan + finish of the host C ABI.  ``raw``: also the filtered counts ``M[keep, ]`` (``$rawCounts``, reference R/gficf.R:40,22)
    as a matrix of its own (own index vectors) — its values gathered by the library's host threads while the results come back
    (``gficf_normalize_csc_host_finish_raw``; behind the multi-GPU finish call: ``gficf_csc_kept_values_host``)."""
    import scipy.sparse as sp

    single = plan is None
    plan = plan or L.gficf_normalize_csc_host_plan
    finish = finish or L.gficf_normalize_csc_host_finish
    gk, nk = ctypes.c_int64(0), ctypes.c_int64(0)
    if w_in is not None:
        w_in = np.ascontiguousarray(w_in, dtype=np.float64)
        if w_in.shape != (G,):
            raise ValueError("w must have one weight per gene (row) of M")
    is64 = 1 if colptr.dtype == np.int64 else 0
    check(plan(ctx.handle, G, N, _np_ptr(colptr), is64, _np_ptr(rowidx), _np_ptr(x),
               float(prop_min), float(prop_max), _np_ptr(w_in), ctypes.byref(gk), ctypes.byref(nk)))
    keep = np.zeros(G, dtype=np.uint8)
    nt = np.zeros(G, dtype=np.int64)
    w = np.zeros(G, dtype=np.float64)
    ocp = np.zeros(N + 1, dtype=colptr.dtype)
    ori = np.empty(nk.value, dtype=np.int32)            # fully written by the finish call
    ox = np.empty(nk.value, dtype=np.float64)
    rri = np.empty(nk.value, dtype=np.int32) if raw else None
    rx = np.empty(nk.value, dtype=np.float64) if raw else None
    if raw and single:
        check(L.gficf_normalize_csc_host_finish_raw(ctx.handle, _np_ptr(keep), _np_ptr(nt), _np_ptr(w), _np_ptr(ocp), _np_ptr(ori), _np_ptr(ox),
                                                    _np_ptr(rowidx), _np_ptr(x), _np_ptr(rri), _np_ptr(rx)))
    else:
        check(finish(ctx.handle, _np_ptr(keep), _np_ptr(nt), _np_ptr(w), _np_ptr(ocp), _np_ptr(ori), _np_ptr(ox)))
        if raw:
            check(L.gficf_csc_kept_values_host(G, N, _np_ptr(colptr), is64, _np_ptr(rowidx), _np_ptr(x), _np_ptr(keep), _np_ptr(ocp),
                                               _np_ptr(rri), _np_ptr(rx)))
    keep = keep.astype(bool)
    out = sp.csc_matrix((ox, ori, ocp), shape=(gk.value, N))
    out.has_sorted_indices = True                        # (M's are — _csc_parts — and the kept rows keep their order: spares later calls scipy's scan)
    if not raw:
        return M, keep, nt, w, out
    if M.dtype != np.float64:
        rx = rx.astype(M.dtype)                          # the counts keep their type, as M[keep, ] does
    rawm = sp.csc_matrix((rx, rri, ocp.copy()), shape=(gk.value, N))
    rawm.has_sorted_indices = True
    return M, keep, nt, w, out, rawm


def tsmessage(*parts, verbose: bool = True, time_stamp: bool = True) -> None:
    """``tsmessage(..., verbose, time_stamp)`` of the reference (R/util.R:30-39): a line on stderr (R's ``message``) behind a
    ``%H:%M:%S`` stamp, nothing when ``verbose`` is false."""
    if verbose:
        import sys
        import time

        print((time.strftime("%H:%M:%S") + " " if time_stamp else "") + "".join(str(p) for p in parts), file=sys.stderr, flush=True)


def gficf(M, cell_proportion_max: float = 1, cell_proportion_min: float = 0.05, storeRaw: bool = True,
          normalize: bool = True, verbose: bool = True, ctx: Context | None = None, *, icf_type: str = "classic",
          norm: str = "l2", devices=None) -> dict:
    """Drop-in for the reference's ``gficf()`` (reference R/gficf.R:17-33).

    ``M``: genes x cells sparse count matrix (scipy CSC — the dgCMatrix analogue).
    Returns the "gficf object" as a dict: ``gficf`` (CSC over the kept genes), ``rawCounts``
    (when ``storeRaw``), ``w`` (ICF weight per kept gene), ``param``; plus ``genes`` (indices
    of the kept genes in M, standing in for R's rownames) and ``nt``.

    ``normalize=TRUE`` in the reference rescales counts with edgeR TMM/CPM
    (R/gficf.R:43-47) before GF; that is a per-cell scale which cancels in x/colSums(x),
    so ``gficf`` is unaffected; with ``normalize=True`` ``rawCounts`` holds the unscaled filtered counts, with a warning.
    ``normalize="tmm"`` runs the rescale on the device (:func:`normCounts`, libgficf_tmm.so): ``rawCounts`` holds the TMM
    counts per million of the kept genes and ``param["normalized"]`` is ``True``; ``gficf`` is the same, bit for bit.

    ``icf_type`` / ``norm`` (keyword only, not arguments of the reference's ``gficf()``, which always runs
    "classic" / "l2") select the other branches of its helpers ``getIdfW(type = ...)`` (R/gficf.R:89-91) and
    ``l.norm(norm = ...)`` (R/gficf.R:100).  ``devices`` (or the environment variable GFICF_HIP_DEVICES): a list of GPUs
    to shard the cells over, single process (``gficf_normalize_csc_host_multi_*``); same result.
    """
    tmm = isinstance(normalize, str)
    if tmm and normalize != "tmm":
        raise ValueError('normalize must be True, False or "tmm"')
    if verbose and normalize and not tmm:
        warnings.warn("normalize=True: the edgeR CPM/TMM rescale (reference R/gficf.R:43-47) is a per-cell scale "
                      "that cancels in the GF step; rawCounts holds unscaled counts (normalize=\"tmm\" runs the rescale on the device)",
                      stacklevel=2)
    # the reference's progress lines (tsmessage: R/gficf.R:58,87,68,99 via R/util.R:30-39; "Normalize counts.." :45 belongs to the
    # edgeR step, which does not run here), same text, on stderr like R's message(); the four steps are ONE device call
    for line in ("Apply GF transformation..", "Compute ICF weigth..", "Applay ICF..", f"Apply {norm}"):
        tsmessage(line, verbose=verbose)
    res = _normalize_csc_host(M, cell_proportion_min, cell_proportion_max, None, ctx, icf_type, norm, devices, raw=storeRaw)
    M, keep, nt, w, out = res[:5]
    data = {"gficf": out}
    if storeRaw:
        data["rawCounts"] = res[5]                        # = M[keep, ] (R/gficf.R:40,22): the result's structure, the counts as values
        if tmm:                                           # cpm(calcNormFactors(DGEList(counts = M[keep, ]))) (R/gficf.R:46), same structure
            tsmessage("Normalize counts..", verbose=verbose)
            data["rawCounts"] = _tmm_host(res[5], want_cpm=True, ctx=ctx)["cpm"]
    data["w"] = w[keep]
    data["genes"] = np.flatnonzero(keep)
    data["nt"] = nt[keep]
    data["param"] = {"cell_proportion_max": cell_proportion_max, "cell_proportion_min": cell_proportion_min,
                     "normalized": True if tmm else normalize}
    return data


def gficf_with_weights(M, w, ctx: Context | None = None):
    """GF -> ICF (weights supplied) -> L2 for new cells (reference R/cellClassifier.R:50-53).

    ``w``: one ICF weight per gene (row) of ``M`` (the R code matches by gene name,
    R/gficf.R:69-78; that name handling stays with the caller).  As in the reference call
    ``normCounts(..., max = 2, min = 0)``, genes absent from every new cell are dropped.
    Returns (gficf CSC over kept genes, kept gene indices).
    """
    _, keep, _, _, out = _normalize_csc_host(M, 0.0, 2.0, w, ctx)
    return out, np.flatnonzero(keep)


def cluster_signatures(gficf_mat, cluster, ctx: Context | None = None):
    """``data$cluster.gene.rnk`` of ``clustcells()`` (reference R/clustCells.R:121-123).

    ``gficf_mat``: the GF-ICF matrix (genes x cells, scipy CSC); ``cluster``: one label per cell.
    Returns (G x C float64 matrix whose column j is the gene-wise sum over the cells of the j-th label,
    labels in order of first appearance — ``base::unique`` order —, and that label list).
    """
    M, colptr, rowidx, x = _csc_parts(gficf_mat)
    G, N = M.shape
    lab = np.asarray(cluster)
    if lab.shape != (N,):
        raise ValueError("cluster must hold one label per cell")
    uniq, first, inv = np.unique(lab, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                 # first-appearance order (R/clustCells.R:122)
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    ids = np.ascontiguousarray(rank[inv], dtype=np.int32)
    C = len(uniq)
    out = np.zeros((C, G), dtype=np.float64)                  # C-order (C, G) == column-major G x C
    ctx = ctx or default_context()
    is64 = 1 if colptr.dtype == np.int64 else 0
    check(_lib.load().gficf_cluster_signatures_host(ctx.handle, G, N, _np_ptr(colptr), is64, _np_ptr(rowidx), _np_ptr(x),
                                                    _np_ptr(ids), C, _np_ptr(out)))
    return out.T, uniq[order]


# ------------------------------------------------------------------ TMM normalisation (libgficf_tmm.so)
def _tmm_host(M, ref_col=None, logratioTrim=.3, sumTrim=.05, doWeighting=True, max_lds_n=0, want_cpm=False, ctx: Context | None = None):
    """``gficf_tmm_host`` on a genes x cells count matrix: the statistics, the reference column, the factors and, with
    ``want_cpm``, the counts per million as a CSC matrix of ``M``'s structure."""
    import scipy.sparse as sp

    from . import _tmm_lib

    M, colptr, rowidx, x = _csc_parts(M)
    G, N = M.shape
    if G < 1 or N < 1:
        raise ValueError("the count matrix must hold at least one gene and one cell")
    for name, v in (("logratioTrim", logratioTrim), ("sumTrim", sumTrim)):
        if not 0 <= float(v) < .5:
            raise ValueError(f"{name} must lie in [0, 0.5)")
    if ref_col is None:
        ref_col = -1
    elif not 0 <= int(ref_col) < N:
        raise ValueError("refColumn must be the (0-based) index of a column of M")
    lib, sq, f75, raw, f = (np.zeros(N, dtype=np.float64) for _ in range(5))
    ostat = np.zeros((2, N), dtype=np.float64)
    n, kept = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    gp, ref = ctypes.c_int32(0), ctypes.c_int64(-1)
    out = np.zeros(max(len(x), 1), dtype=np.float64) if want_cpm else None
    ctx = ctx or default_context()
    check(_tmm_lib.load().gficf_tmm_host(ctx.handle, G, N, _np_ptr(colptr), 1 if colptr.dtype == np.int64 else 0, _np_ptr(rowidx), _np_ptr(x), int(ref_col),
                                         float(logratioTrim), float(sumTrim), 1 if doWeighting else 0, int(max_lds_n), None, None, _np_ptr(lib), _np_ptr(sq),
                                         _np_ptr(f75), _np_ptr(ostat), ctypes.byref(gp), ctypes.byref(ref), _np_ptr(raw), _np_ptr(f), _np_ptr(n), _np_ptr(kept),
                                         _np_ptr(out)))
    res = {"norm.factors": f, "lib.size": lib, "refColumn": int(ref.value), "f75": f75, "n": n, "kept": kept, "sq": sq, "ostat": ostat,
           "Gprime": int(gp.value), "factors.raw": raw}
    if want_cpm:
        X = sp.csc_matrix((out[:len(x)], rowidx.copy(), colptr.copy()), shape=(G, N))
        X.has_sorted_indices = True
        res["cpm"] = X
    return res


def calcNormFactors(M, refColumn=None, logratioTrim: float = .3, sumTrim: float = .05, doWeighting: bool = True, max_lds_n: int = 0,
                    ctx: Context | None = None) -> dict:
    """edgeR's ``calcNormFactors(DGEList(counts = M), method = "TMM")`` on the device, from the sparse matrix (the
    ``normalize = TRUE`` branch of the reference, R/gficf.R:46), under the contract of include/gficf_tmm.h: the trim ranks on
    ``obs / ref`` and ``obs * ref``, which tie exactly where the genes are mathematically tied (the tie rule).

    ``M``: genes x cells counts (scipy sparse); ``refColumn``: the 0-based index of the reference column, or ``None`` for
    edgeR's choice.  Returns ``norm.factors`` (their geometric mean is 1), ``lib.size`` (the column sums), ``refColumn``,
    ``f75`` (the upper-quartile factor of every column), ``n`` and ``kept`` (the common genes of every cell and the
    reference, and how many of them survive the trim); also ``sq``, ``ostat``, ``Gprime`` and ``factors.raw`` (the stages).
    ``max_lds_n`` lowers the LDS capacity beyond which a cell is ranked by the counting kernel (0: the library's)."""
    return _tmm_host(M, refColumn, logratioTrim, sumTrim, doWeighting, max_lds_n, False, ctx)


def cpm(M, lib_size=None, norm_factors=None, ctx: Context | None = None):
    """edgeR's ``cpm(M, lib.size, norm.factors)``: ``x / (1e-6 * (lib.size * norm.factors))`` on the device, as a CSC
    matrix of ``M``'s structure (never dense).  ``lib_size=None``: the column sums; ``norm_factors=None``: ones."""
    import scipy.sparse as sp

    from . import _tmm_lib

    M, colptr, rowidx, x = _csc_parts(M)
    G, N = M.shape
    if G < 1 or N < 1:
        raise ValueError("the count matrix must hold at least one gene and one cell")
    f = np.ones(N, dtype=np.float64) if norm_factors is None else np.ascontiguousarray(norm_factors, dtype=np.float64)
    lib = None if lib_size is None else np.ascontiguousarray(lib_size, dtype=np.float64)
    if f.shape != (N,) or (lib is not None and lib.shape != (N,)):
        raise ValueError("lib_size and norm_factors must hold one value per cell")
    out = np.zeros(max(len(x), 1), dtype=np.float64)
    ctx = ctx or default_context()
    check(_tmm_lib.load().gficf_tmm_host(ctx.handle, G, N, _np_ptr(colptr), 1 if colptr.dtype == np.int64 else 0, _np_ptr(rowidx), _np_ptr(x), -1, .3, .05,
                                         1, 0, _np_ptr(lib), _np_ptr(f), None, None, None, None, None, None, None, None, None, None, _np_ptr(out)))
    X = sp.csc_matrix((out[:len(x)], rowidx.copy(), colptr.copy()), shape=(G, N))
    X.has_sorted_indices = True
    return X


def _norm_counts(M, doc_proportion_max, doc_proportion_min, normalizeCounts, verbose, ctx):
    """:func:`normCounts`, and the mask of the rows it keeps."""
    import scipy.sparse as sp

    M = sp.csr_matrix(M)
    N = M.shape[1]
    ix = np.diff((M != 0).tocsr().indptr)
    keep = (ix > N * doc_proportion_min) & (ix <= N * doc_proportion_max)
    M = sp.csc_matrix(M[keep])
    if normalizeCounts:
        tsmessage("Normalize counts..", verbose=verbose)
        M = _tmm_host(M, want_cpm=True, ctx=ctx)["cpm"]
    return M, keep


def normCounts(M, doc_proportion_max: float = 1, doc_proportion_min: float = .01, normalizeCounts: bool = False, verbose: bool = True,
               ctx: Context | None = None):
    """``normCounts(M, doc_proportion_max, doc_proportion_min, normalizeCounts, verbose)`` of the reference (R/gficf.R:38-50):
    the genes found in more than ``doc_proportion_min`` and at most ``doc_proportion_max`` of the cells and, with
    ``normalizeCounts``, their TMM counts per million (:func:`calcNormFactors`, :func:`cpm`), sparse."""
    return _norm_counts(M, doc_proportion_max, doc_proportion_min, normalizeCounts, verbose, ctx)[0]


# ------------------------------------------------------------------ marker genes (libgficf_markers.so)
def _first_appearance_ids(cluster, N: int):
    """Labels numbered in order of first appearance (``base::unique`` order): (int32 ids, the label list)."""
    lab = np.asarray(cluster)
    if lab.shape != (N,):
        raise ValueError("cluster must hold one label per cell")
    uniq, first, inv = np.unique(lab, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    return np.ascontiguousarray(rank[inv], dtype=np.int32), uniq[order]


def cluster_markers(cpms_csc, cluster, ctx: Context | None = None):
    """One-vs-rest Mann-Whitney U test of every gene for every cluster, the test inside ``findClusterMarkers()`` (reference
    R/deGenes.R:43-48 -> ``rcpp_parallel_WMU_test(cpms[, in], cpms[, out])``), all clusters in one call.

    ``cpms_csc``: genes x cells (scipy sparse); ``cluster``: one label per cell.  Returns ``(P, LFC, labels)``: G x C float64
    p-values and log2 fold changes, column j for the j-th label in ``base::unique`` order (``labels``).  The arithmetic is
    the reference's, quirks included (include/gficf_markers.h).
    """
    from . import _markers_lib

    M, colptr, rowidx, x = _csc_parts(cpms_csc)
    G, N = M.shape
    ids, labels = _first_appearance_ids(cluster, N)
    C = len(labels)
    P = np.zeros((C, G), dtype=np.float64)                   # C-order (C, G) == column-major G x C
    LFC = np.zeros((C, G), dtype=np.float64)
    ctx = ctx or default_context()
    is64 = 1 if colptr.dtype == np.int64 else 0
    check(_markers_lib.load().gficf_cluster_markers_host(ctx.handle, G, N, _np_ptr(colptr), is64, _np_ptr(rowidx), _np_ptr(x),
                                                         _np_ptr(ids), C, _np_ptr(P), _np_ptr(LFC)))
    return P.T, LFC.T, labels


def rcpp_parallel_WMU_test(matX, matY, printOutput: bool = False, ctx: Context | None = None) -> np.ndarray:
    """``rcpp_parallel_WMU_test(matX, matY, printOutput)`` (reference src/rcpp_parallel_mann_whitney.cpp:107-129): per row, the
    Mann-Whitney U test of matX's row against matY's.  Returns G x 2: ``[p, log2FC]``."""
    from . import _markers_lib

    X = np.asfortranarray(matX, dtype=np.float64)
    Y = np.asfortranarray(matY, dtype=np.float64)
    if X.ndim != 2 or Y.ndim != 2 or X.shape[0] != Y.shape[0]:
        raise ValueError("matX and matY must be matrices with the same number of rows")
    G = X.shape[0]
    out = np.zeros((2, G), dtype=np.float64)                # C-order (2, G) == column-major G x 2
    if printOutput:
        print("Running Parallell WM-U test...")
    ctx = ctx or default_context()
    check(_markers_lib.load().gficf_cluster_markers_dense_host(ctx.handle, G, X.shape[1], _np_ptr(X), Y.shape[1], _np_ptr(Y), _np_ptr(out)))
    if printOutput:
        print("Done!!")
    return out.T


def rcpp_WMU_test(M, idx1, idx2, ctx: Context | None = None) -> np.ndarray:
    """``rcpp_WMU_test(M, idx1, idx2)`` (reference src/rcpp_mann_whitney.cpp): the same test between the columns ``idx1`` and
    ``idx2`` of ``M`` (1-based, as the reference's ``subset()`` takes them).  Returns G x 2: ``[p, log2FC]``."""
    M = np.asarray(M, dtype=np.float64)
    i1 = np.asarray(idx1, dtype=np.int64) - 1
    i2 = np.asarray(idx2, dtype=np.int64) - 1
    if M.ndim != 2 or ((i1 < 0) | (i1 >= M.shape[1])).any() or ((i2 < 0) | (i2 >= M.shape[1])).any():
        raise ValueError("idx1 / idx2 must be 1-based column indices of M")
    return rcpp_parallel_WMU_test(M[:, i1], M[:, i2], False, ctx)


def p_adjust_fdr(p) -> np.ndarray:
    """R's ``p.adjust(p, method = "fdr")`` (Benjamini-Hochberg), in R's order of operations:
    ``pmin(1, cummin(n / i * p[o]))[ro]`` with ``o = order(p, decreasing = TRUE)``."""
    p = np.asarray(p, dtype=np.float64)
    n = len(p)
    if n == 0:
        return p.copy()
    i = np.arange(n, 0, -1, dtype=np.float64)
    o = np.argsort(-p, kind="stable")
    q = np.minimum(1.0, np.minimum.accumulate((n / i) * p[o]))
    out = np.empty(n, dtype=np.float64)
    out[o] = q
    return out


# ------------------------------------------------------------------ highly variable genes (libgficf_hvg.so)
def _hvg_outputs(G: int, stages: bool) -> dict:
    from . import _hvg_lib

    o = {k: np.full(G, np.nan, dtype=np.float64) for k in ("lx", "ly", "fit", "weights", "cvDist", "P")}
    o["valid"] = np.zeros(G, dtype=np.int32)
    o["scalars"] = np.full(len(_hvg_lib.SCALARS), np.nan, dtype=np.float64)
    if stages:
        o["g5"], o["ySeq"] = np.zeros(_hvg_lib.GRID5_MAX, dtype=np.float64), np.zeros(_hvg_lib.GRID5_MAX, dtype=np.float64)
        o["gap"] = np.zeros(_hvg_lib.GRID5_MAX, dtype=np.int32)
    return o


def _hvg_result(o: dict, mean, cv, stages: bool) -> dict:
    """The outputs of the host entries as the dictionary of :func:`var_genes_from_moments`."""
    from . import _hvg_lib

    sc = dict(zip(_hvg_lib.SCALARS, o["scalars"]))
    valid = o["valid"] != 0
    fdr = np.full(len(valid), np.nan, dtype=np.float64)
    fdr[valid] = p_adjust_fdr(o["P"][valid])
    r = {"mean": mean, "cv": cv, "P": o["P"], "FDR": fdr}
    if stages:
        n5 = int(sc["len5"])
        r.update({k: o[k] for k in ("lx", "ly", "fit", "weights", "cvDist")})
        r.update({"valid": valid, "s": np.array([sc["s0"], sc["s1"], sc["s2"]]), "g5": o["g5"][:n5].copy(), "gap": o["gap"][:n5].copy(),
                  "ySeq": o["ySeq"][:n5].copy()})
        r.update({k: int(sc[k]) for k in ("n", "k", "cdx0", "j0", "nls_iter")})
        r.update({k: float(sc[k]) for k in ("b", "a", "bw", "distMid", "mu", "sigma")})
    return r


def _hvg_enough(n_valid: int) -> None:
    if int(np.floor(0.2 * n_valid)) < 4:
        raise ValueError(f"{n_valid} genes with a finite log10 mean and log10 cv: the local regression needs at least 20")


def gene_moments(M, ctx: Context | None = None) -> dict:
    """Per-gene moments of the genes x cells matrix ``M`` (scipy sparse, at least 2 cells) in one pass over its stored entries
    (step 1 of include/gficf_hvg.h): ``mean``, ``sd`` and ``var`` (the n - 1 denominator, two passes as R's ``sd``), ``nobs``
    (the stored non-zeros), and ``lx = log10(mean)``, ``ly = log10(sd / mean)``, ``valid`` (both finite)."""
    from . import _hvg_lib

    M, colptr, rowidx, x = _csc_parts(M)
    G, N = M.shape
    if G < 1 or N < 2:
        raise ValueError("the matrix must hold at least one gene and two cells")
    mean, sd, var, lx, ly = (np.zeros(G, dtype=np.float64) for _ in range(5))
    nobs, valid = np.zeros(G, dtype=np.int32), np.zeros(G, dtype=np.int32)
    ctx = ctx or default_context()
    check(_hvg_lib.load().gficf_hvg_host(ctx.handle, G, N, _np_ptr(colptr), 1 if colptr.dtype == np.int64 else 0, _np_ptr(rowidx), _np_ptr(x), 1,
                                         _np_ptr(mean), _np_ptr(sd), _np_ptr(var), _np_ptr(nobs), _np_ptr(lx), _np_ptr(ly), _np_ptr(valid), None, None,
                                         None, None, None, None, None, None))
    return {"mean": mean, "sd": sd, "var": var, "nobs": nobs, "lx": lx, "ly": ly, "valid": valid != 0}


def var_genes_from_moments(mean, cv, ctx: Context | None = None) -> dict:
    """Steps 2 - 7 of :func:`findVarGenes` from the genes' ``mean`` and ``cv`` (include/gficf_hvg.h): the robust local
    regression of log10 cv on log10 mean, the trusted range, the curve ``0.5 * log10(b / x + a)``, the signed distances, their
    mode and the p-values.  Returns every stage: ``lx, ly, valid, fit, weights, s`` (3), ``g5, gap, ySeq, cdx0, j0, b, a,
    nls_iter, cvDist, bw, distMid, mu, sigma, P, FDR`` (per-gene arrays hold NaN at the invalid genes), and ``n``, ``k``."""
    from . import _hvg_lib

    mean, cv = np.ascontiguousarray(mean, dtype=np.float64), np.ascontiguousarray(cv, dtype=np.float64)
    if mean.ndim != 1 or mean.shape != cv.shape or len(mean) < 1:
        raise ValueError("mean and cv must be vectors of one length")
    with np.errstate(divide="ignore", invalid="ignore"):
        _hvg_enough(int((np.isfinite(np.log10(mean)) & np.isfinite(np.log10(cv))).sum()))
    o = _hvg_outputs(len(mean), True)
    ctx = ctx or default_context()
    check(_hvg_lib.load().gficf_hvg_trend_host(ctx.handle, len(mean), _np_ptr(mean), _np_ptr(cv), _np_ptr(o["lx"]), _np_ptr(o["ly"]), _np_ptr(o["valid"]),
                                               _np_ptr(o["fit"]), _np_ptr(o["weights"]), _np_ptr(o["cvDist"]), _np_ptr(o["P"]), _np_ptr(o["scalars"]),
                                               _np_ptr(o["g5"]), _np_ptr(o["gap"]), _np_ptr(o["ySeq"])))
    return _hvg_result(o, mean, cv, True)


def findVarGenes(cpms, fitMethod: str = "locfit", verbose: bool = True, genes=None, ret_stages: bool = False, ctx: Context | None = None):
    """``findVarGenes(data, fitMethod, verbose)`` of the reference (R/deGenes.R:72-164; scVEGs, Chen et al. 2016) on the
    device, from the sparse matrix, under the contract of include/gficf_hvg.h.  ``cpms``: the normalised genes x cells
    counts.  Returns a ``pandas.DataFrame`` with the columns ``gene, mean, cv, P, FDR``, one row per row of ``cpms`` in its
    order (``gene``: ``genes``, or the row index); a gene without a finite log10 mean and log10 cv has NaN in P and FDR.
    ``ret_stages=True``: a dictionary with those columns and every stage of :func:`var_genes_from_moments`, and ``sd``,
    ``var``, ``nobs``.  Only ``fitMethod="locfit"`` (the one ``findClusterMarkers`` uses) is provided."""
    from . import _hvg_lib

    if fitMethod != "locfit":
        raise NotImplementedError(f'fitMethod="{fitMethod}" is not provided: only "locfit", the fit findClusterMarkers() asks for')
    M, colptr, rowidx, x = _csc_parts(cpms)
    G, N = M.shape
    if N < 2:
        raise ValueError("the standard deviation of a gene needs at least 2 cells")
    if genes is not None and len(genes) != G:
        raise ValueError("genes must hold one name per row of cpms")
    _hvg_enough(G)
    o = _hvg_outputs(G, ret_stages)
    mean, sd, var = (np.zeros(G, dtype=np.float64) for _ in range(3))
    nobs = np.zeros(G, dtype=np.int32)
    ctx = ctx or default_context()
    check(_hvg_lib.load().gficf_hvg_host(ctx.handle, G, N, _np_ptr(colptr), 1 if colptr.dtype == np.int64 else 0, _np_ptr(rowidx), _np_ptr(x), 0,
                                         _np_ptr(mean), _np_ptr(sd), _np_ptr(var), _np_ptr(nobs), _np_ptr(o["lx"]), _np_ptr(o["ly"]), _np_ptr(o["valid"]),
                                         _np_ptr(o["fit"]), _np_ptr(o["weights"]), _np_ptr(o["cvDist"]), _np_ptr(o["P"]), _np_ptr(o["scalars"]),
                                         _np_ptr(o.get("g5")), _np_ptr(o.get("gap")), _np_ptr(o.get("ySeq"))))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = _hvg_result(o, mean, sd / mean, ret_stages)
    r["gene"] = np.arange(G) if genes is None else np.asarray(genes)
    if ret_stages:
        r.update({"sd": sd, "var": var, "nobs": nobs})
        return r
    import pandas as pd

    return pd.DataFrame({k: r[k] for k in ("gene", "mean", "cv", "P", "FDR")})


def _hvg_vectors(*arrays):
    out = [np.ascontiguousarray(a, dtype=np.float64) for a in arrays]
    if any(a.ndim != 1 or a.shape != out[0].shape for a in out) or len(out[0]) < 1:
        raise ValueError("the arguments must be vectors of one length")
    if not all(np.isfinite(a).all() for a in out):
        raise ValueError("the arguments must be finite")
    return out


def local_regression(x, y, at=None, nn: float = 0.2, weights=None, robust_iter: int = 0, ret_h: bool = False, device: int = 0):
    """The local regression of :func:`findVarGenes` on its own (step 2 of include/gficf_hvg.h; locfit's ``lp(x, nn)`` at
    ``deg = 2`` with the tricube kernel, every value a direct fit): ``y`` on ``x`` over the ``floor(nn * n)`` nearest points,
    evaluated at ``at`` (``None``: at ``x``).  ``weights``: prior weights of the points; ``robust_iter``: rounds of
    Cleveland's bisquare reweighting before the returned fit (``locfit.robust`` runs 3).  ``ret_h=True``: also the bandwidth
    at every evaluation point."""
    x, y = _hvg_vectors(x, y)
    n = len(x)
    k = int(np.floor(nn * n))
    if not 1 <= k <= n:
        raise ValueError("nn must leave between 1 and all of the points in a window")
    wv = None
    if weights is not None:
        (wv,) = _hvg_vectors(weights)
        if wv.shape != x.shape or (wv < 0).any():
            raise ValueError("weights must hold one non-negative value per point")
    if at is not None:
        (at,) = _hvg_vectors(at)
    ops = _umap_hip(device)
    tc = ops.torch
    dev = tc.device("cuda", device)
    t = lambda v: tc.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev)
    d_x = t(x)
    ws = tc.empty(ops.hvg_workspace_bytes(n), dtype=tc.uint8, device=dev)
    perm, count = tc.empty(n, dtype=tc.int32, device=dev), tc.empty(1, dtype=tc.int32, device=dev)
    ops.hvg_order(d_x, None, ws, perm, count)
    perm = perm.long()
    xs, ys = d_x[perm].contiguous(), t(y)[perm].contiguous()
    w = None if wv is None else t(wv)[perm].contiguous()
    if robust_iter > 0:
        w_out, f_n, s = tc.empty(n, dtype=tc.float64, device=dev), tc.empty(n, dtype=tc.float64, device=dev), tc.empty(int(robust_iter), dtype=tc.float64, device=dev)
        ops.hvg_robust(xs, ys, k, int(robust_iter), ws, w_out, f_n, s, w_in=w)
        w = w_out
    d_at = d_x if at is None else t(at)
    fit, h = tc.empty(d_at.numel(), dtype=tc.float64, device=dev), tc.empty(d_at.numel(), dtype=tc.float64, device=dev)
    ops.hvg_locfit(xs, ys, w, k, d_at, ws, fit, h)
    ops.hvg_sync(ws)
    return (fit.cpu().numpy(), h.cpu().numpy()) if ret_h else fit.cpu().numpy()


def curve_distance(lx, ly, b: float, a: float, ret_index: bool = False, device: int = 0):
    """Step 5 of :func:`findVarGenes` on its own: the signed distance ``cvDist`` of every gene ``(lx, ly)`` to the curve
    ``0.5 * log10(b / 10^g + a)`` on the grid ``g = seq(min lx, max lx, 0.001)``.  ``ret_index=True``: also the index of the
    nearest grid point."""
    lx, ly = _hvg_vectors(lx, ly)
    x0 = float(lx.min())
    glen = int(np.floor((float(lx.max()) - x0) / 0.001 + 1e-10)) + 1
    ops = _umap_hip(device)
    tc = ops.torch
    dev = tc.device("cuda", device)
    ws = tc.empty(ops.hvg_workspace_bytes(len(lx), grid_pts=glen), dtype=tc.uint8, device=dev)
    out, idx = tc.empty(len(lx), dtype=tc.float64, device=dev), tc.empty(len(lx), dtype=tc.int32, device=dev)
    ops.hvg_curve_distance(tc.from_numpy(lx).to(dev), tc.from_numpy(ly).to(dev), b, a, x0, glen, ws, out, idx)
    ops.hvg_sync(ws)
    return (out.cpu().numpy(), idx.cpu().numpy()) if ret_index else out.cpu().numpy()


def hvg_rows(fdr) -> np.ndarray:
    """The rows ``findClusterMarkers(hvg = TRUE)`` keeps, in its order (R/deGenes.R:31-35): ordered stably by FDR (NaN last),
    those with FDR < .1 or, if they are at most 1000, the first ``min(1000, G)``."""
    fdr = np.asarray(fdr, dtype=np.float64)
    o = np.argsort(fdr, kind="stable")
    sig = int((fdr[o] < .1).sum())
    return o[:sig] if sig > 1000 else o[:min(1000, len(o))]


def findClusterMarkers(data: dict, nt: int = 2, hvg=True, verbose: bool = True, cpms=None, ctx: Context | None = None) -> dict:
    """``findClusterMarkers(data, nt, hvg, verbose)`` of the reference (R/deGenes.R:15-60): marker genes of every cluster, the
    Mann-Whitney U test of each cluster against the rest on the device (``cluster_markers``), then the reference's R
    post-processing: per cluster in ``unique`` order ``fdr = p.adjust(p, "fdr")``, keep ``fdr < .05 & log2FC > 0``, order by
    fdr, ``rbind``; the whole table ordered by log2FC, decreasing (both orders stable).  ``data$de.genes`` becomes a
    ``pandas.DataFrame`` with the columns ``ens, log2FC, p.value, fdr, cluster``.

    ``cpms``: the normalised genes x cells matrix (rows as ``data["rawCounts"]``), or ``"tmm"`` for the reference's own
    ``normCounts(rawCounts, 2, 0, !normalized)`` (R/deGenes.R:25) on the device (:func:`normCounts`).  Without ``cpms`` the
    raw counts are tested, with a warning.  Genes
    with no non-zero cell are dropped first (``normCounts(doc_proportion_min = 0)``); the rest set BH's n.  ``hvg="locfit"``
    runs the reference's selection (R/deGenes.R:27-37) with :func:`findVarGenes` on the device: the genes ordered by FDR, those
    below 10 % or, if they are at most 1000, the first 1000, tested in that order.  ``hvg=True`` stands for the reference's
    own locfit fit (at kd-tree vertices, interpolated), which is not provided: pass ``hvg="locfit"`` (every value a direct
    fit), ``hvg=False``, or an array of the row indices to keep.
    ``nt`` is accepted for signature compatibility.  ``ens`` holds ``data["genes"]`` of the kept rows (the stand-in for R's
    rownames) or, without it, the row indices.
    """
    import pandas as pd
    import scipy.sparse as sp

    if data.get("community") is None:
        raise ValueError("Please identify cluster first! Run clustcells function.")
    if data.get("rawCounts") is None:
        raise ValueError("No raw/normalized counts stored. You should have run gficf normalization with storeRaw = T")
    if hvg is True:
        raise NotImplementedError("hvg=True is the reference's locfit fit at kd-tree vertices, which is not provided: pass "
                                  "hvg=\"locfit\" for findVarGenes with every value a direct fit (include/gficf_hvg.h), hvg=False, or the "
                                  "row indices of the genes to keep")
    if isinstance(hvg, str) and hvg != "locfit":
        raise ValueError('hvg must be "locfit", False or the row indices of the genes to keep')
    kept_rows = None
    if isinstance(cpms, str):
        if cpms != "tmm":
            raise ValueError('cpms must be a matrix, None or "tmm"')
        cpms, kept_rows = _norm_counts(data["rawCounts"], 2, 0, not (data.get("param") or {}).get("normalized", False), verbose, ctx)
    elif cpms is None:
        warnings.warn("findClusterMarkers: no cpms= given, the raw counts are tested (the edgeR rescale is not run here; cpms=\"tmm\" "
                      "runs it on the device)", stacklevel=2)
        cpms = data["rawCounts"]
    M = sp.csr_matrix(cpms)
    names = np.asarray(data["genes"]) if data.get("genes") is not None and len(data["genes"]) == M.shape[0] else np.arange(M.shape[0])
    if kept_rows is not None and not kept_rows.all():        # normCounts dropped rows: the names follow
        names = np.asarray(data["genes"])[kept_rows] if data.get("genes") is not None and len(data["genes"]) == len(kept_rows) else np.flatnonzero(kept_rows)
    if isinstance(hvg, str):                                 # R/deGenes.R:27-37 on the rows normCounts(doc_proportion_min = 0) leaves
        tsmessage("... Detecting HVGs", verbose=verbose)
        left = np.flatnonzero(np.diff((M != 0).tocsr().indptr) > 0)
        fdr = findVarGenes(M[left], verbose=verbose, ctx=ctx)["FDR"].to_numpy()
        tsmessage(f"... Detected {int((fdr < .1).sum())} significant HVGs with an FDR < 10%", verbose=verbose)
        rows = left[hvg_rows(fdr)]
    else:
        rows = np.arange(M.shape[0]) if hvg is False or hvg is None else np.asarray(hvg, dtype=np.int64)
    M = M[rows]
    keep = np.diff((M != 0).tocsr().indptr) > 0             # normCounts(doc_proportion_min = 0): rowSums(M != 0) > 0
    rows, M = rows[keep], sp.csc_matrix(M[keep])
    cl = data.get("cluster")
    if cl is None:
        cl = np.asarray(data["community"]).astype(str)
    tsmessage("... Start identify marker genes", verbose=verbose)
    P, LFC, labels = cluster_markers(M, cl, ctx)
    parts = []
    for j, lab in enumerate(labels):
        fdr = p_adjust_fdr(P[:, j])
        sel = np.flatnonzero((fdr < .05) & (LFC[:, j] > 0))
        sel = sel[np.argsort(fdr[sel], kind="stable")]
        parts.append(pd.DataFrame({"ens": names[rows[sel]], "log2FC": LFC[sel, j], "p.value": P[sel, j], "fdr": fdr[sel],
                                   "cluster": np.repeat(lab, len(sel))}))
    res = pd.concat(parts, ignore_index=True)
    res = res.iloc[np.argsort(-res["log2FC"].to_numpy(), kind="stable")].reset_index(drop=True)
    data["de.genes"] = res
    return data


# ------------------------------------------------------------------ pathways (libgficf_gsea.so)
def gmt_pathways(gmt_file, convertToEns: bool = False, convertHu2Mm: bool = False, verbose: bool = True, gene_map=None) -> dict:
    """``gmtPathways(gmt.file, convertToEns, convertHu2Mm, verbose)`` of the reference (R/pathwayAnalisys.R:2-42): every line of
    the gmt file split on tabs, field 1 the name, field 2 dropped, the rest the members; pathways left without a member are
    dropped.  Returns ``{name: [members]}`` in file order (of a repeated name the first line is kept).

    The reference converts the symbols through biomaRt, which needs the network.  Here, with either flag true, ``gene_map`` (a
    dict from symbol to a list of ids, or to one id) does that mapping: a pathway becomes the ids of its members, unique with
    order kept, unmapped members and missing ids dropped.  A flag without ``gene_map`` raises ``NotImplementedError``.
    """
    if (convertToEns or convertHu2Mm) and gene_map is None:
        raise NotImplementedError("convertToEns / convertHu2Mm look the genes up through biomaRt, which is not provided: pass "
                                  "gene_map={symbol: [ids]}")
    pathways = {}
    with open(gmt_file) as f:
        for line in f:
            fields = line.rstrip("\r\n").split("\t")
            while fields and fields[-1] == "":                # strsplit drops the trailing empty field
                fields.pop()
            if fields and fields[0] not in pathways:
                pathways[fields[0]] = fields[2:]
    if convertToEns or convertHu2Mm:
        what = ("human symbols to mouse ensamble id" if convertToEns else "human symbols to mouse symbols") if convertHu2Mm \
            else "human symbols to human ensamble id"
        tsmessage(f".. Start converting {what}", verbose=verbose)
        for name, members in pathways.items():
            ids = []
            for sym in members:
                hit = gene_map.get(sym, [])
                ids.extend([hit] if isinstance(hit, str) else hit)
            pathways[name] = list(dict.fromkeys(i for i in ids if i is not None and i == i))
        tsmessage("Done!", verbose=verbose)
    return {name: members for name, members in pathways.items() if len(members) > 0}


def gsea(stats, pathways_ptr, pathways_rows, nsim: int = 1000, min_size=1, max_size=np.inf, seed: int = 180582, ret_null: bool = False,
         ctx: Context | None = None, *, exact: bool = False) -> dict:
    """Gene-set enrichment of every column of ``stats`` (G x C, one ranking statistic per gene and cluster) for P pathways in
    CSR form (``pathways_ptr``: P + 1 offsets, ``pathways_rows``: rows of ``stats``), fgsea at ``gseaParam = 0`` under the
    relaxed contract of include/gficf_gsea.h: ES and NES are fgsea's, the p-value is ``fgseaSimple``'s estimator over ``nsim``
    permutations (never below ``1 / (nsim + 1)``), one null per set size shared by all clusters.

    Returns ``es``, ``nes``, ``pval`` (P x C; zeros where a pathway is not tested), ``size`` (P), ``tested`` (P; size within
    ``[min_size, min(max_size, G - 1)]``) and, with ``ret_null``, ``sizes`` (the D distinct tested sizes) and ``null`` (D x nsim).

    ``exact=True`` (off by default: the sweep costs far more than the sampled call) adds two P x C outputs that have no
    permutation floor (include/gficf_gsea_exact.h; the others keep their bits).  ``ptail``: the exact one-sided tail of ES under
    the uniform null of the set's size, :func:`gsea_tail`; 0 where a pathway is not tested, 1 where ES is 0.  ``pval_exact =
    min(1, ptail * (nsim + 1) / (n0 + 1))`` with ``n0`` the number of null values of that size that are ``>= 0`` when ES > 0 and
    ``<= 0`` when ES < 0 (counted on the host in the null table the call makes anyway), and 1 when ES is 0: the exact one-sided
    tail divided by a sampled probability of the sign.  It is at least the limit of the simple estimator's numerator
    ``P(ES >= x)``; the two differ by ``P(maxP >= x, -minP >= maxP)``, negligible once p is small.  A set larger than
    ``GFICF_GSEA_EXACT_MAX_SIZE`` has a NaN ``ptail`` and keeps ``pval`` as its ``pval_exact`` (one warning).
    """
    from . import _gsea_lib

    S = np.asarray(stats, dtype=np.float64)
    if S.ndim == 1:
        S = S[:, None]
    if S.ndim != 2 or S.shape[0] < 1 or S.shape[1] < 1:
        raise ValueError("stats must be a G x C matrix")
    G, C = S.shape
    S = np.ascontiguousarray(S.T)                            # C-order (C, G) == column-major G x C
    ptr = np.ascontiguousarray(pathways_ptr, dtype=np.int64)
    rows = np.ascontiguousarray(pathways_rows, dtype=np.int32)
    if ptr.ndim != 1 or len(ptr) < 1 or ptr[0] != 0 or (np.diff(ptr) < 0).any() or rows.ndim != 1 or ptr[-1] != len(rows):
        raise ValueError("pathways_ptr must hold P + 1 non-decreasing offsets from 0 to len(pathways_rows)")
    if int(nsim) < 1:
        raise ValueError("nsim must be at least 1")
    P, nsim = len(ptr) - 1, int(nsim)
    size = np.diff(ptr)
    lo, hi = int(max(min_size, 1)), int(min(max_size, G - 1))
    tested = (size >= lo) & (size <= hi)
    sizes = np.unique(size[tested])
    es, nes, pval = (np.zeros((C, P), dtype=np.float64) for _ in range(3))
    null = np.zeros((len(sizes), nsim), dtype=np.float64) if ret_null or exact else None
    ctx = ctx or default_context()
    check(_gsea_lib.load().gficf_gsea_host(ctx.handle, G, C, _np_ptr(S), P, _np_ptr(ptr), _np_ptr(rows), nsim, int(seed) & 0xFFFFFFFF, lo, hi,
                                           _np_ptr(es), _np_ptr(nes), _np_ptr(pval), _np_ptr(null) if null is not None else None, len(sizes)))
    out = {"es": es.T, "nes": nes.T, "pval": pval.T, "size": size, "tested": tested}
    if ret_null:
        out["sizes"], out["null"] = sizes, null
    if exact:
        out["ptail"], out["pval_exact"] = _gsea_exact_pvalues(G, size, tested, sizes, null, out["es"], out["pval"], nsim, ctx)
    return out


def gsea_tail(G: int, size, es, ctx: Context | None = None) -> np.ndarray:
    """The exact one-sided tail of enrichment scores at ``gseaParam = 0`` (include/gficf_gsea_exact.h): for every pair of a set
    size ``m`` in ``[1, G - 1]`` and a score ``x`` as :func:`gsea` returns it, the share of the m-subsets of G positions with
    ``maxP >= x`` (x > 0) or ``minP <= x`` (x < 0); 1 for x == 0.  A lattice-path count in f64, relative error at most
    ``4 G 2^-52`` down to 1e-290; NaN for a size above ``GFICF_GSEA_EXACT_MAX_SIZE``.  ``size`` and ``es`` broadcast against each
    other; the result has their shape."""
    from . import _gsea_exact_lib

    size, es = np.broadcast_arrays(np.asarray(size), np.asarray(es, dtype=np.float64))
    if size.size and (size.dtype.kind not in "iu" or np.abs(size).max() > np.iinfo(np.int32).max):
        raise ValueError("size must hold int32 set sizes")
    if int(G) < 2:
        raise ValueError("G must be at least 2")
    shape = size.shape
    m = np.ascontiguousarray(size, dtype=np.int32).ravel()
    x = np.ascontiguousarray(es, dtype=np.float64).ravel()
    tail = np.zeros(len(m), dtype=np.float64)
    ctx = ctx or default_context()
    check(_gsea_exact_lib.load().gficf_gsea_tail_host(ctx.handle, int(G), len(m), _np_ptr(m), _np_ptr(x), _np_ptr(tail)))
    return tail.reshape(shape)


def _gsea_exact_pvalues(G, size, tested, sizes, null, es, pval, nsim, ctx):
    """``ptail`` and ``pval_exact`` of :func:`gsea` (P x C) from its ES, its null table and its simple p-values."""
    from . import _gsea_exact_lib

    t = np.flatnonzero(tested)
    ptail, pexact = np.zeros_like(es), np.zeros_like(es)
    if len(t) == 0:
        return ptail, pexact
    e = es[t]
    ptail[t] = gsea_tail(G, size[t][:, None], e, ctx)
    d = np.searchsorted(sizes, size[t])
    n_ge, n_le = (null >= 0).sum(axis=1)[d], (null <= 0).sum(axis=1)[d]
    n0 = np.where(e > 0, n_ge[:, None], n_le[:, None]).astype(np.float64)
    pe = np.minimum(1.0, ptail[t] * np.float64(nsim + 1) / (n0 + 1.0))
    pe[e == 0] = 1.0
    over = np.isnan(ptail[t])
    if over.any():
        import warnings

        warnings.warn(f"{int(over.any(axis=1).sum())} pathways hold more than GFICF_GSEA_EXACT_MAX_SIZE = {_gsea_exact_lib.MAX_SIZE} genes: their "
                      "pval_exact is the simple estimator's pval")
        pe[over] = pval[t][over]
    pexact[t] = pe
    return ptail, pexact


def _pathway_csr(pathways: dict, gene_names):
    """The members of every pathway matched to the rows named ``gene_names`` (fgsea's ``fmatch``: the first row of a name),
    unmatched ones dropped, made unique with order kept: (ptr, rows)."""
    row_of = {}
    for i, g in enumerate(gene_names):
        row_of.setdefault(str(g), i)
    ptr, rows = [0], []
    for members in pathways.values():
        rows.extend(dict.fromkeys(row_of[str(m)] for m in members if str(m) in row_of))
        ptr.append(len(rows))
    return np.asarray(ptr, dtype=np.int64), np.asarray(rows, dtype=np.int32)


def fgsea(pathways: dict, stats, nsim: int = 1000, minSize=1, maxSize=np.inf, seed: int = 180582, names=None, ctx: Context | None = None, *,
          exact: bool = False):
    """``fgsea(pathways, stats, minSize, maxSize, gseaParam = 0)`` for one ranked vector: ``stats`` is a ``pandas.Series`` indexed
    by gene name, or an array plus ``names``.  Returns a ``pandas.DataFrame`` ``pathway, pval, padj, ES, NES, size`` of the tested
    pathways in input order; ``padj = p.adjust(pval, "BH")`` over them.  Relaxed contract: see :func:`gsea`.  ``exact=True``:
    ``pval`` and ``padj`` come from ``pval_exact`` of :func:`gsea`, and the simple estimator's is kept as the column ``pval_simple``."""
    import pandas as pd

    if names is None:
        if not isinstance(stats, pd.Series):
            raise ValueError("stats must be a pandas Series indexed by gene name, or an array with names=")
        names = stats.index
    v = np.asarray(stats, dtype=np.float64)
    if v.ndim != 1 or len(names) != len(v):
        raise ValueError("stats must hold one value per name")
    ptr, rows = _pathway_csr(pathways, names)
    r = gsea(v, ptr, rows, nsim, minSize, maxSize, seed, False, ctx, exact=bool(exact))
    t = np.flatnonzero(r["tested"])
    pv = r["pval_exact" if exact else "pval"][t, 0]
    out = pd.DataFrame({"pathway": [n for n, k in zip(pathways, r["tested"]) if k], "pval": pv, "padj": p_adjust_fdr(pv), "ES": r["es"][t, 0],
                        "NES": r["nes"][t, 0], "size": r["size"][t]})
    if exact:
        out["pval_simple"] = r["pval"][t, 0]
    return out


def runGSEA(data: dict, gmt_file=None, nsim: int = 1000, convertToEns: bool = False, convertHu2Mm: bool = False, nt: int = 2, minSize=15,
            maxSize=np.inf, verbose: bool = True, seed: int = 180582, method: str = "GSEA", *, pathways=None, gene_names=None, gene_map=None,
            ctx: Context | None = None, exact: bool = False) -> dict:
    """``runGSEA(data, gmt.file, nsim, convertToEns, convertHu2Mm, nt, minSize, maxSize, verbose, seed, method)`` of the
    reference (R/pathwayAnalisys.R:65-96): gene-set enrichment of every cluster's ``data["cluster.gene.rnk"]`` column, all
    clusters in one device call (:func:`gsea`; the reference calls ``fgseaMultilevel(..., gseaParam = 0)`` per cluster).

    ``pathways``: a dict ``{name: [genes]}`` in place of ``gmt_file`` (read by :func:`gmt_pathways`, with ``gene_map`` for the
    conversions).  ``gene_names``: one name per row of ``data["gficf"]``; default ``data["gene_names"]``, else
    ``data["genes"]`` as strings.  Members are matched by name, made unique, unmatched ones dropped, as fgsea does.
    ``convertToEns`` defaults to False here (True in the reference, where it asks biomaRt): the one default that differs.
    ``nt`` is accepted for signature compatibility.  ``method="GSVA"`` (GSVA / limma) is :func:`runGSVA`'s.

    ``data["gsea"]`` becomes ``{"pathways", "es", "nes", "pval", "fdr", "stat"}``: the four tables are ``pandas.DataFrame``
    (index: pathway names, columns: ``data["cluster.labels"]``) holding zeros where a pathway was not tested, ``fdr`` is
    Benjamini-Hochberg per cluster over the tested pathways, ``stat`` lists ``pathway, size`` of the tested pathways.
    Relaxed contract (include/gficf_gsea.h): ES and NES are fgsea's; the p-value is ``fgseaSimple``'s with ``nsim``
    permutations, not the multilevel estimate; the random bits are this library's.  ``exact=True`` adds the tables ``ptail``,
    ``pval_exact`` (see :func:`gsea`: the exact one-sided tail over a sampled probability of the sign, no floor at
    ``1 / (nsim + 1)``) and ``fdr_exact``, Benjamini-Hochberg of ``pval_exact`` per cluster over the tested pathways; ``pval`` and
    ``fdr`` stay the simple estimator's.
    """
    import pandas as pd

    if data.get("cluster.gene.rnk") is None:
        raise ValueError("Please run clustcell function first")
    if method not in ("GSEA", "GSVA"):
        raise ValueError("'method' should be one of \"GSEA\", \"GSVA\"")
    if method == "GSVA":
        raise NotImplementedError("method=\"GSVA\" (GSVA scores and limma models) is a function of its own: call runGSVA")
    tsmessage("Choosen method is GSEA...", verbose=verbose)
    if pathways is None:
        if gmt_file is None:
            raise ValueError("give gmt_file or pathways=")
        pathways = gmt_pathways(gmt_file, convertToEns, convertHu2Mm, verbose, gene_map)
    else:
        pathways = {str(k): list(v) for k, v in pathways.items() if len(v) > 0}
    stats = np.asarray(data["cluster.gene.rnk"], dtype=np.float64)
    if gene_names is None:
        gene_names = data.get("gene_names")
    if gene_names is None and data.get("genes") is not None:
        gene_names = np.asarray(data["genes"]).astype(str)
    if gene_names is None or len(gene_names) != stats.shape[0]:
        raise ValueError("gene_names must hold one name per row of data[\"cluster.gene.rnk\"]")
    labels = data.get("cluster.labels")
    labels = list(range(stats.shape[1])) if labels is None else list(labels)
    ptr, rows = _pathway_csr(pathways, gene_names)
    tsmessage(f"GSEA of {len(pathways)} pathways in {stats.shape[1]} clusters, {int(nsim)} permutations", verbose=verbose)
    r = gsea(stats, ptr, rows, nsim, minSize, maxSize, seed, False, ctx, exact=bool(exact))
    t = np.flatnonzero(r["tested"])
    cols = [("es", r["es"]), ("nes", r["nes"]), ("pval", r["pval"])]
    for key, pv in (("fdr", r["pval"]),) + ((("fdr_exact", r["pval_exact"]),) if exact else ()):
        fdr = np.zeros_like(pv)
        for c in range(stats.shape[1]):
            fdr[t, c] = p_adjust_fdr(pv[t, c])
        cols.append((key, fdr))
    if exact:
        cols += [("ptail", r["ptail"]), ("pval_exact", r["pval_exact"])]
    names = list(pathways)
    tab = {k: pd.DataFrame(v, index=names, columns=labels) for k, v in cols}
    data["gsea"] = {"pathways": pathways, **tab,
                    "stat": pd.DataFrame({"pathway": [names[i] for i in t], "size": r["size"][t]})}
    tsmessage("Done!", verbose=verbose)
    return data


# ------------------------------------------------------------------ GSVA and its limma contrasts (libgficf_gsva.so)
def _gsva_args(M, cluster, ptr, members, min_size, max_size, n_clusters):
    """What :func:`gsva` and :func:`gsva_scores` decide before the first call into the library: the gene-major CSR (canonical:
    duplicates summed, columns ascending, stored zeros kept), the int32 cluster ids, C, the pathway CSR and the size bounds."""
    import scipy.sparse as sp

    M = sp.csr_matrix(M)
    if M.dtype != np.float64:
        M = M.astype(np.float64)
    if not M.has_canonical_format:
        M = M.copy()
        M.sum_duplicates()
    G, N = M.shape
    if G < 1 or N < 1:
        raise ValueError("gficf must be a genes x cells matrix with at least one gene and one cell")
    cl = np.asarray(cluster)
    if cl.shape != (N,) or not np.issubdtype(cl.dtype, np.integer):
        raise ValueError("cluster must hold one integer id per cell")
    cl = np.ascontiguousarray(cl, dtype=np.int32)
    C = int(n_clusters) if n_clusters is not None else max(int(cl.max()) + 1, 1)
    if C < 1:
        raise ValueError("n_clusters must be at least 1")
    ptr = np.ascontiguousarray(ptr, dtype=np.int64)
    members = np.ascontiguousarray(members, dtype=np.int32)
    if ptr.ndim != 1 or len(ptr) < 1 or ptr[0] != 0 or (np.diff(ptr) < 0).any() or members.ndim != 1 or ptr[-1] != len(members):
        raise ValueError("ptr must hold P + 1 non-decreasing offsets from 0 to len(members)")
    if min_size != min_size or max_size != max_size:
        raise ValueError("min_size and max_size must not be NaN")
    lo, hi = int(max(min_size, 1)), int(min(max_size, G))
    return M, cl, C, ptr, members, lo, hi


def _gsva_cell_major(rows, cols, N: int):
    """The cell-major form of entries given gene-major (``rows`` ascending): (colptr, row, src) with ``src`` the index of
    each entry in the gene-major arrays."""
    src = np.lexsort((rows, cols)).astype(np.int64)
    colptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=N), out=colptr[1:])
    return colptr, np.ascontiguousarray(rows[src], dtype=np.int32), src


def _gsva_forms(M, cl, C: int):
    """The two sparse forms include/gficf_gsva.h asks for, from the canonical gene-major CSR ``M`` and the cluster ids: the
    entries grouped by (gene, cluster) (seg_ptr, cell, x; ``perm`` maps a grouped position to its CSR position) and the same
    entries cell-major (colptr, row, src)."""
    G, N = M.shape
    rows = np.repeat(np.arange(G, dtype=np.int64), np.diff(M.indptr))
    cols = M.indices.astype(np.int64)
    seg = rows * C + np.clip(cl[cols], 0, C - 1)            # an id out of range is the library's to reject
    perm = np.argsort(seg, kind="stable")                    # cells stay ascending within a segment
    seg_ptr = np.zeros(G * C + 1, dtype=np.int64)
    np.cumsum(np.bincount(seg, minlength=G * C), out=seg_ptr[1:])
    cell = np.ascontiguousarray(cols[perm], dtype=np.int32)
    x = np.ascontiguousarray(M.data[perm], dtype=np.float64)
    colptr, row, src = _gsva_cell_major(rows[perm], cols[perm], N)
    return seg_ptr, cell, x, perm, colptr, row, src


def _gsva_out(es, tested, ssum, ssq):
    """The outputs both host entries share, from their column-major arrays."""
    return {"es": es.T, "tested": tested.T.astype(bool), "sum": ssum.T, "sumsq": ssq.T}


def gsva(gficf, cluster, ptr, members, min_size=1, max_size=np.inf, ret_stages: bool = False, n_clusters=None, ctx: Context | None = None) -> dict:
    """GSVA scores of every cell within its cluster (``GSVA::gsva(gficf[, cells], pathways, kcdf="Gaussian", method="gsva")``
    of the reference's ``runGSEA(method="GSVA")``, R/pathwayAnalisys.R:113) for all clusters in one device call, under the
    contract of include/gficf_gsva.h: the Gaussian kernel CDF is evaluated exactly, not from GSVA's table.

    ``gficf``: genes x cells (scipy sparse, stored zeros allowed); ``cluster``: one integer id in ``[0, C)`` per cell
    (``n_clusters``: C, default ``max + 1``); pathways in CSR form (``ptr``: P + 1 offsets, ``members``: rows).

    Returns ``es`` (P x N; zeros where a pathway is not tested in the cell's cluster), ``tested`` (P x C), ``kept`` (G x C: the
    genes that pass GSVA's constant-gene filter in the cluster), ``sum`` and ``sumsq`` (P x C: the sums of ``es`` and of its
    squares over each cluster's cells, computed on the device for :func:`gsva_de_pathways`).  With ``ret_stages`` also ``sd``,
    ``d0`` (G x C) and ``d_nz``, the density of every stored entry in the CSR order of ``scipy.sparse.csr_matrix(gficf)``."""
    from . import _gsva_lib

    M, cl, C, ptr, members, lo, hi = _gsva_args(gficf, cluster, ptr, members, min_size, max_size, n_clusters)
    G, N = M.shape
    P = len(ptr) - 1
    seg_ptr, cell, x, perm, colptr, row, src = _gsva_forms(M, cl, C)
    es = np.zeros((N, P), dtype=np.float64)                  # C-order (N, P) == column-major P x N
    tested = np.zeros((C, P), dtype=np.int32)
    ssum, ssq = np.zeros((C, P), dtype=np.float64), np.zeros((C, P), dtype=np.float64)
    kept = np.zeros((C, G), dtype=np.int32)
    sd, d0 = np.zeros((C, G), dtype=np.float64), np.zeros((C, G), dtype=np.float64)
    dnz = np.zeros(max(len(x), 1), dtype=np.float64)
    ctx = ctx or default_context()
    check(_gsva_lib.load().gficf_gsva_host(ctx.handle, G, N, C, _np_ptr(cl), _np_ptr(seg_ptr), _np_ptr(cell), _np_ptr(x), _np_ptr(colptr), _np_ptr(row),
                                           _np_ptr(src), P, _np_ptr(ptr), _np_ptr(members), lo, hi, _np_ptr(es), _np_ptr(tested), _np_ptr(kept),
                                           _np_ptr(sd), _np_ptr(d0), _np_ptr(dnz), _np_ptr(ssum), _np_ptr(ssq)))
    out = _gsva_out(es, tested, ssum, ssq)
    out["kept"] = kept.T.astype(bool)
    if ret_stages:
        d_csr = np.zeros(len(x), dtype=np.float64)
        d_csr[perm] = dnz[:len(x)]
        out.update(sd=sd.T, d0=d0.T, d_nz=d_csr)
    return out


def gsva_scores(d_nz, d0, kept, gficf_pattern, cluster, ptr, members, min_size=1, max_size=np.inf, n_clusters=None,
                ctx: Context | None = None) -> dict:
    """Stages 3-5 of :func:`gsva` alone, from given densities: the order of every cell's genes, the tested pathways and the
    scores.  ``d_nz``: one density per stored entry of ``gficf_pattern`` (genes x cells; only its pattern is read) in its CSR
    order; ``d0`` (G x C): the density of a gene's zeros in a cluster; ``kept`` (G x C).  Returns ``es``, ``tested``, ``sum``,
    ``sumsq`` as :func:`gsva` does."""
    from . import _gsva_lib

    M, cl, C, ptr, members, lo, hi = _gsva_args(gficf_pattern, cluster, ptr, members, min_size, max_size, n_clusters)
    G, N = M.shape
    P = len(ptr) - 1
    dnz = np.ascontiguousarray(d_nz, dtype=np.float64)
    d0 = np.asarray(d0, dtype=np.float64)
    kept = np.asarray(kept)
    if dnz.shape != (M.nnz,) or d0.shape != (G, C) or kept.shape != (G, C):
        raise ValueError("d_nz must hold one density per stored entry, d0 and kept must be G x C")
    d0 = np.ascontiguousarray(d0.T)                          # C-order (C, G) == column-major G x C
    kept = np.ascontiguousarray(kept.T != 0, dtype=np.int32)
    rows = np.repeat(np.arange(G, dtype=np.int64), np.diff(M.indptr))
    colptr, row, src = _gsva_cell_major(rows, M.indices.astype(np.int64), N)
    if len(dnz) == 0:
        dnz = np.zeros(1, dtype=np.float64)
    es = np.zeros((N, P), dtype=np.float64)
    tested = np.zeros((C, P), dtype=np.int32)
    ssum, ssq = np.zeros((C, P), dtype=np.float64), np.zeros((C, P), dtype=np.float64)
    ctx = ctx or default_context()
    check(_gsva_lib.load().gficf_gsva_scores_host(ctx.handle, G, N, C, _np_ptr(cl), _np_ptr(colptr), _np_ptr(row), _np_ptr(src), M.nnz, _np_ptr(dnz),
                                                  _np_ptr(d0), _np_ptr(kept), P, _np_ptr(ptr), _np_ptr(members), lo, hi, _np_ptr(es), _np_ptr(tested),
                                                  _np_ptr(ssum), _np_ptr(ssq)))
    return _gsva_out(es, tested, ssum, ssq)


def _trigamma_inverse(x: float) -> float:
    """The y with ``trigamma(y) = x`` by Newton's iteration on ``1 / trigamma`` (limma's ``trigammaInverse``)."""
    from scipy.special import polygamma

    if x > 1e7:
        return 1.0 / np.sqrt(x)
    if x < 1e-6:
        return 1.0 / x
    y = 0.5 + 1.0 / x
    for _ in range(50):
        tri = float(polygamma(1, y))
        dif = tri * (1.0 - tri / x) / float(polygamma(2, y))
        y += dif
        if -dif / y < 1e-8:
            break
    return y


def _squeeze_var(s2: np.ndarray, df: float):
    """limma's ``squeezeVar`` in the plain form (no covariate, not robust): the prior ``(s0², df0)`` by ``fitFDist``'s moments
    of ``log s²`` and the posterior variances."""
    from scipy.special import digamma, polygamma

    n = len(s2)
    if n == 1:
        return s2.copy(), float(s2[0]), 0.0
    v = np.maximum(s2, 0.0)
    m = np.median(v)
    if m == 0:
        m = 1.0
    v = np.maximum(v, 1e-5 * m)
    e = np.log(v) - digamma(df / 2.0) + np.log(df / 2.0)
    emean = e.mean()
    evar = ((e - emean) ** 2).sum() / (n - 1) - float(polygamma(1, df / 2.0))
    if evar > 0:
        df0 = 2.0 * _trigamma_inverse(float(evar))
        s02 = float(np.exp(emean + digamma(df0 / 2.0) - np.log(df0 / 2.0)))
        return (df * s2 + df0 * s02) / (df + df0), s02, df0
    s02 = float(v.mean())
    return np.full(n, s02), s02, np.inf


def gsva_de_pathways(res: dict, cluster, labels=None, names=None, cluster_minus_other: bool = False):
    """The limma step of the reference's ``runGSEA(method="GSVA")`` (R/pathwayAnalisys.R:118-136) from what :func:`gsva`
    returned: for every cluster, ``lmFit`` of the scores on cluster-against-the-rest, ``eBayes`` and ``topTable``, finished on
    the host in float64 from the per-cluster sums the device computed (``res["sum"]``, ``res["sumsq"]``).

    Rows: the pathways whose scores are not all zero (a positive sum of squares; a pathway with a NaN score, W = 0 in the
    header, has no finite sums and is left out).  Returns a DataFrame ``logFC, AveExpr,
    t, P.Value, adj.P.Val, pathway, cluster``, the clusters in id order (``labels[c]`` names cluster c, ``names[p]`` pathway p),
    each cluster's rows by decreasing ``|t|`` (topTable's order by ``B``, which is monotone in ``t²`` here).  ``logFC`` is
    mean(other) - mean(cluster), the sign the reference's ``model.matrix(~ factor(clusters))`` gives its ``C<label>vsOTHER``
    coefficient (the level ``C<label>`` sorts before ``other``); ``cluster_minus_other=True`` flips it (and ``t``).  ``eBayes`` is
    the non-robust form without trend; the ``B`` column (limma's ``tmixture`` prior) is not provided."""
    import pandas as pd
    from scipy import stats

    if not isinstance(res, dict) or "sum" not in res or "sumsq" not in res:
        raise ValueError("res must be what gsva() or gsva_scores() returned (the device's sums are read from it)")
    S, Q = np.asarray(res["sum"], dtype=np.float64), np.asarray(res["sumsq"], dtype=np.float64)
    P, C = S.shape
    cl = np.asarray(cluster)
    n1 = np.bincount(cl, minlength=C).astype(np.float64)
    N = float(len(cl))
    use = np.flatnonzero(Q.sum(axis=1) > 0)
    labels = list(range(C)) if labels is None else list(labels)
    names = np.arange(P) if names is None else np.asarray(names)
    cols = ["logFC", "AveExpr", "t", "P.Value", "adj.P.Val", "pathway", "cluster"]
    if len(use) == 0 or N < 3:
        return pd.DataFrame({k: [] for k in cols})
    St, Qt = S[use].sum(axis=1), Q[use].sum(axis=1)
    parts = []
    df = N - 2.0
    for c in range(C):
        a, b = n1[c], N - n1[c]
        if a < 1 or b < 1:
            continue
        S1, S2 = S[use, c], St - S[use, c]
        rss = np.maximum((Q[use, c] - S1 * S1 / a) + ((Qt - Q[use, c]) - S2 * S2 / b), 0.0)
        s2 = rss / df
        coef = S2 / b - S1 / a
        post, _, df0 = _squeeze_var(s2, df)
        t = coef / (np.sqrt(1.0 / a + 1.0 / b) * np.sqrt(post))
        dft = min(df + df0, len(use) * df)
        pv = 2.0 * stats.t.sf(np.abs(t), dft)
        if cluster_minus_other:
            coef, t = -coef, -t
        o = np.argsort(-np.abs(t), kind="stable")
        parts.append(pd.DataFrame({"logFC": coef[o], "AveExpr": (St / N)[o], "t": t[o], "P.Value": pv[o], "adj.P.Val": p_adjust_fdr(pv)[o],
                                   "pathway": names[use][o], "cluster": np.repeat(labels[c], len(o))}))
    return pd.concat(parts, ignore_index=True) if parts else pd.DataFrame({k: [] for k in cols})


def runGSVA(data: dict, gmt_file=None, minSize=15, maxSize=np.inf, pathways=None, gene_names=None, convertToEns: bool = False, gene_map=None,
            nt: int = 2, verbose: bool = True, *, convertHu2Mm: bool = False, cluster_minus_other: bool = False, ctx: Context | None = None) -> dict:
    """The ``method="GSVA"`` branch of the reference's ``runGSEA`` (R/pathwayAnalisys.R:97-138): GSVA scores of every cell
    within its cluster (:func:`gsva`, all clusters in one device call) and one limma contrast per cluster on the score matrix
    (:func:`gsva_de_pathways`).  The clusters are ``data["cluster"]`` in ``unique`` order; pathways and gene names are read as
    :func:`runGSEA` reads them.  ``nt`` is accepted for signature compatibility.

    ``data["gsva"]`` becomes ``{"pathways", "res", "DEpathways"}``: ``res`` a DataFrame pathways x cells without the rows that
    are zero everywhere, ``DEpathways`` the limma table ``logFC, AveExpr, t, P.Value, adj.P.Val, pathway, cluster``.  Differences
    from GSVA and limma (include/gficf_gsva.h): the kernel CDF is exact, there is no ``B`` column, and ``logFC`` keeps the
    reference's sign, mean(other) - mean(cluster), unless ``cluster_minus_other=True``."""
    import pandas as pd

    if data.get("gficf") is None:
        raise ValueError("Please run gficf function first")
    if data.get("cluster") is None:
        raise ValueError("Please run clustcell function first")
    tsmessage("Choosen method is GSVA...", verbose=verbose)
    if pathways is None:
        if gmt_file is None:
            raise ValueError("give gmt_file or pathways=")
        pathways = gmt_pathways(gmt_file, convertToEns, convertHu2Mm, verbose, gene_map)
    else:
        pathways = {str(k): list(v) for k, v in pathways.items() if len(v) > 0}
    M = data["gficf"]
    if gene_names is None:
        gene_names = data.get("gene_names")
    if gene_names is None and data.get("genes") is not None:
        gene_names = np.asarray(data["genes"]).astype(str)
    if gene_names is None or len(gene_names) != M.shape[0]:
        raise ValueError("gene_names must hold one name per row of data[\"gficf\"]")
    ids, labels = _first_appearance_ids(data["cluster"], M.shape[1])
    ptr, rows = _pathway_csr(pathways, gene_names)
    tsmessage(f"Start executiong GSVA: {len(pathways)} pathways, {len(labels)} clusters", verbose=verbose)
    r = gsva(M, ids, ptr, rows, minSize, maxSize, False, len(labels), ctx)
    names = np.asarray(list(pathways))
    use = (r["es"] != 0).any(axis=1)                         # rowSums(res != 0) > 0
    tsmessage("Start executiong Limma cluster by cluster", verbose=verbose)
    data["gsva"] = {"pathways": pathways,
                    "res": pd.DataFrame(r["es"][use], index=names[use]),
                    "DEpathways": gsva_de_pathways(r, ids, labels, names, cluster_minus_other)}
    tsmessage("Done!", verbose=verbose)
    return data


def run_modularity_clustering(SNN, modularity: int = 1, resolution: float = 0.8, algorithm: int = 1, n_start: int = 10,
                              n_iter: int = 10, random_seed: int = 0, print_output: bool = False, ctx: Context | None = None):
    """``RunModularityClustering(SNN, modularity, resolution, algorithm, n.start, n.iter, random.seed, print.output)``
    (reference R/clustCells.R:145-149 -> src/RModularityOptimizer.cpp:25) on the symmetric weighted adjacency matrix of
    the Jaccard graph (``jaccard_adjacency``).  RELAXED CONTRACT (see include/gficf_hip.h): a deterministic parallel
    Louvain on the reference's objective — standard modularity with a resolution parameter, diagonal ignored — instead
    of its sequential, seeded one.  ``n_start`` starts each begin from singletons and the best modularity is kept, as in the
    reference; what a start varies is the seed (from ``random_seed`` and the start number) of the hash that splits the
    vertices into sub-round classes — the result is a function of the arguments, never of scheduling.  ``modularity`` 1 (standard) or 2 (alternative: unit node weights, resolution <= 1), ``algorithm`` 1 (Louvain) or 2
    (Louvain with multilevel refinement).

    ``SNN`` must be symmetric (the reference reads its strict lower triangle and mirrors it).

    Returns the cluster of every vertex (int32, 0-based like the reference's return value, clusters numbered by
    decreasing size); ``.modularity`` and ``.n_clusters`` are attached as attributes of the returned array subclass.
    """
    import scipy.sparse as sp

    if modularity not in (1, 2):
        raise ValueError("Modularity parameter must be equal to 1 or 2.")
    if modularity == 2 and resolution > 1.0:
        raise ValueError("error: resolution<1 for alternative modularity")
    if algorithm not in (1, 2):
        raise ValueError("algorithm must be 1 (Louvain) or 2 (Louvain with multilevel refinement); algorithm 3 (smart local moving) is slm()")
    if n_start < 1 or n_iter < 1:
        raise ValueError("n_start and n_iter must be at least 1")
    A = sp.csc_matrix(SNN)
    if A.shape[0] != A.shape[1]:
        raise ValueError("SNN must be square")
    if not A.has_sorted_indices:
        A = A.copy()
        A.sort_indices()
    N = A.shape[0]
    indptr = np.ascontiguousarray(A.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(A.indices, dtype=np.int32)
    x = np.ascontiguousarray(A.data, dtype=np.float64)
    labels = np.zeros(max(N, 1), dtype=np.int32)
    nc, q = ctypes.c_int64(0), ctypes.c_double(0.0)
    ctx = ctx or default_context()
    L = _lib.load()
    check(L.gficf_ctx_set_louvain_options(ctx.handle, int(modularity)))
    try:
        check(L.gficf_louvain_host(ctx.handle, N, _np_ptr(indptr), 1, _np_ptr(indices), _np_ptr(x), float(resolution), int(algorithm),
                                   int(n_start), int(n_iter), int(random_seed) & 0x7FFFFFFF, _np_ptr(labels), ctypes.byref(nc), ctypes.byref(q)))
    finally:
        L.gficf_ctx_set_louvain_options(ctx.handle, 1)
    out = labels[:N].view(ClusterLabels)
    out.modularity, out.n_clusters = q.value, nc.value
    if print_output:
        print(f"Number of nodes: {N}\nModularity: {q.value:.4f}\nNumber of communities: {nc.value}")
    return out


class ClusterLabels(np.ndarray):
    """int32 labels with the modularity and cluster count of the run attached."""
    modularity = float("nan")
    n_clusters = 0
    n_edges = 0



def _leiden_matrix(A, resolution):
    """The checks of ``leiden`` / ``leiden_refine`` that need no device, and the matrix as the C ABI takes it."""
    import scipy.sparse as sp

    if not (np.isfinite(resolution) and resolution >= 0.0):
        raise ValueError("resolution must be finite and not negative")
    A = sp.csc_matrix(A)
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise ValueError("the adjacency matrix must be square")
    if not A.has_sorted_indices:
        A = A.copy()
        A.sort_indices()
    return (A.shape[0], np.ascontiguousarray(A.indptr, dtype=np.int64), np.ascontiguousarray(A.indices, dtype=np.int32),
            np.ascontiguousarray(A.data, dtype=np.float64))


def _leiden_labels(labels, N, what):
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    if lab.shape != (N,):
        raise ValueError(f"{what} must hold one label per vertex ({N}), not {lab.shape}")
    if N and (lab.min() < 0 or lab.max() >= N):
        raise ValueError(f"{what} labels must lie in [0, {N})")
    return lab


def leiden(A, resolution: float = 1.0, n_iterations: int = 2, seed: int = 0, init=None, ctx: Context | None = None):
    """Leiden community detection (Traag, Waltman, van Eck 2019) on a symmetric weighted adjacency matrix, what
    ``clustcells(community.algo = "leiden")`` of the reference runs (R/clustCells.R:100-107,
    ``leiden::leiden(object = g, resolution_parameter = resolution)``).

    RELAXED CONTRACT (include/gficf_leiden.h): the algorithm and its objective are Leiden's — the modularity of
    :func:`run_modularity_clustering` with a resolution, local moving, refinement into well-connected sub-communities,
    aggregation by the refined partition — the visiting order and the random bits are not leidenalg's; the refinement takes
    the target of largest gain where leidenalg draws one at random.  Every community returned is connected.  The result is
    a function of the arguments, bit for bit.  ``init``: a start partition (labels in [0, N)); ``n_iterations`` >= 1:
    each further iteration resumes from the last one's result.

    Returns ``ClusterLabels`` (int32, 0-based, clusters numbered by decreasing size) with ``.modularity`` and ``.n_clusters``.
    """
    from . import _leiden_lib

    if n_iterations < 1:
        raise ValueError("n_iterations must be at least 1")
    N, indptr, indices, x = _leiden_matrix(A, resolution)
    start = None if init is None else _leiden_labels(init, N, "init")
    labels = np.zeros(max(N, 1), dtype=np.int32)
    nc, q = ctypes.c_int64(0), ctypes.c_double(0.0)
    ctx = ctx or default_context()
    check(_leiden_lib.load().gficf_leiden_host(ctx.handle, N, _np_ptr(indptr), _np_ptr(indices), _np_ptr(x), len(indices), float(resolution),
                                               int(n_iterations), int(seed) & 0x7FFFFFFF, None if start is None else _np_ptr(start),
                                               _np_ptr(labels), ctypes.byref(nc), ctypes.byref(q)))
    out = labels[:N].view(ClusterLabels)
    out.modularity, out.n_clusters = q.value, nc.value
    return out


def leiden_refine(A, labels, resolution: float = 1.0, ctx: Context | None = None):
    """The refinement stage of :func:`leiden` alone: every community of ``labels`` split into connected, well-connected
    sub-communities (include/gficf_leiden.h).  Returns int32[N]: the smallest member id of every vertex's refined community."""
    from . import _leiden_lib

    N, indptr, indices, x = _leiden_matrix(A, resolution)
    lab = _leiden_labels(labels, N, "labels")
    out = np.zeros(max(N, 1), dtype=np.int32)
    nr = ctypes.c_int64(0)
    ctx = ctx or default_context()
    check(_leiden_lib.load().gficf_leiden_refine_host(ctx.handle, N, _np_ptr(indptr), _np_ptr(indices), _np_ptr(x), len(indices), float(resolution),
                                                      _np_ptr(lab), _np_ptr(out), ctypes.byref(nr)))
    return out[:N]


def slm(A, resolution: float = 0.8, n_start: int = 10, n_iter: int = 10, seed: int = 0, init=None, ctx: Context | None = None):
    """The smart local moving algorithm (Waltman, van Eck 2013) on a symmetric weighted adjacency matrix: ``algorithm = 3`` of the
    reference's ``RunModularityClustering`` (src/ModularityOptimizer.cpp:651-690), as a function of its own.

    RELAXED CONTRACT (include/gficf_slm.h): the algorithm and its objective are SLM's — the level loop of :func:`leiden` with a
    full local moving inside every community, from singletons, where Leiden merges singletons once — the visiting order and the
    random bits are not the reference's.  ``n_start`` runs with seeds ``seed + s``, the one of largest modularity returned (ties:
    the first); ``n_iter`` iterations each, fewer when an iteration returns its own start.  The result is a function of the
    arguments, bit for bit.  ``init``: a start partition (labels in [0, N)).

    Returns ``ClusterLabels`` (int32, 0-based, clusters numbered by decreasing size) with ``.modularity``, ``.n_clusters``,
    ``.start`` (the start the result came from) and ``.iterations`` (how many that start ran).
    """
    from . import _slm_lib

    if n_start < 1 or n_iter < 1:
        raise ValueError("n_start and n_iter must be at least 1")
    N, indptr, indices, x = _leiden_matrix(A, resolution)
    start = None if init is None else _leiden_labels(init, N, "init")
    labels = np.zeros(max(N, 1), dtype=np.int32)
    info = _slm_lib.Info()
    ctx = ctx or default_context()
    check(_slm_lib.load().gficf_slm_host(ctx.handle, N, _np_ptr(indptr), _np_ptr(indices), _np_ptr(x), len(indices), float(resolution),
                                         int(n_start), int(n_iter), int(seed) & 0xFFFFFFFF, None if start is None else _np_ptr(start),
                                         _np_ptr(labels), ctypes.byref(info)))
    out = labels[:N].view(ClusterLabels)
    out.modularity, out.n_clusters, out.start, out.iterations = info.modularity, info.n_clusters, info.start, info.iterations
    return out


def slm_submove(A, labels, resolution: float = 1.0, seed: int = 0, level: int = 0, ctx: Context | None = None):
    """The sub-moving stage of :func:`slm` alone on the finest graph: local moving from singletons inside every community of
    ``labels`` (include/gficf_slm.h, step 3).  Returns int32[N], the smallest member id of every vertex's sub-community, with
    ``.n_clusters`` (their number) and ``.passes``."""
    from . import _slm_lib

    if level < 0:
        raise ValueError("level must not be negative")
    N, indptr, indices, x = _leiden_matrix(A, resolution)
    lab = _leiden_labels(labels, N, "labels")
    out = np.zeros(max(N, 1), dtype=np.int32)
    info = _slm_lib.SubmoveInfo()
    ctx = ctx or default_context()
    check(_slm_lib.load().gficf_slm_submove_host(ctx.handle, N, _np_ptr(indptr), _np_ptr(indices), _np_ptr(x), len(indices), float(resolution),
                                                 _np_ptr(lab), int(seed) & 0xFFFFFFFF, int(level), _np_ptr(out), ctypes.byref(info)))
    out = out[:N].view(ClusterLabels)
    out.n_clusters, out.passes = info.n_sub, info.passes
    return out


def transpose_gficf(gficf_mat, ctx: Context | None = None):
    """``data$pca$cells = t(data$gficf)`` (reference R/dimensinalityReduction.R:33, :100): the genes x cells CSC
    matrix as a cells x genes CSC matrix (cell indices ascending within every gene, every stored entry kept)."""
    import scipy.sparse as sp

    M, colptr, rowidx, x = _csc_parts(gficf_mat)
    G, N = M.shape
    nnz = len(rowidx)
    out_ptr = np.zeros(G + 1, dtype=np.int64)
    out_idx = np.zeros(max(nnz, 1), dtype=np.int32)
    out_x = np.zeros(max(nnz, 1), dtype=np.float64)
    ctx = ctx or default_context()
    is64 = 1 if colptr.dtype == np.int64 else 0
    check(_lib.load().gficf_csc_transpose_host(ctx.handle, G, N, _np_ptr(colptr), is64, _np_ptr(rowidx), _np_ptr(x),
                                               _np_ptr(out_ptr), _np_ptr(out_idx), _np_ptr(out_x)))
    T = sp.csc_matrix((out_x[:nnz], out_idx[:nnz], out_ptr), shape=(N, G))
    T.has_sorted_indices = True
    return T


# ------------------------------------------------------------------ PCA / LSA (libgficf_pca.so)
RSVD_MAX_L = 128


def csc_tmm(A_csc, X, ctx: Context | None = None) -> np.ndarray:
    """``t(A) %*% X`` for a sparse ``A`` (nrows x ncols, scipy CSC) and a dense ``X`` (nrows x l, l <= 128): ncols x l.  The
    building block of :func:`rsvd` and of :func:`pca_project` (``gficf_csc_tmm_host``)."""
    from . import _pca_lib

    M, colptr, rowidx, x = _csc_parts(A_csc)
    nrows, ncols = M.shape
    X = np.asfortranarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] != nrows:
        raise ValueError("X must be a matrix with one row per row of A")
    l = X.shape[1]
    Y = np.zeros((l, ncols), dtype=np.float64)                # C-order (l, ncols) == column-major ncols x l
    ctx = ctx or default_context()
    is64 = 1 if colptr.dtype == np.int64 else 0
    check(_pca_lib.load().gficf_csc_tmm_host(ctx.handle, nrows, ncols, _np_ptr(colptr), is64, _np_ptr(rowidx), _np_ptr(x), _np_ptr(X), l, _np_ptr(Y)))
    return Y.T


def rsvd(A_csc_genes_x_cells, k: int, p: int = 10, q: int = 2, seed: int = 180582, omega=None, centre: bool = False,
         ctx: Context | None = None) -> dict:
    """``rsvd::rsvd(t(M), k, p = 10, q = 2)`` / the decomposition inside ``rsvd::rpca`` for the genes x cells matrix ``M``
    (scipy CSC): the randomized SVD of the cells x genes matrix ``A = t(M)``, with ``centre`` of ``A`` minus its column means
    (never densified).  RELAXED CONTRACT (include/gficf_pca.h): the algorithm is rsvd's, its bits are not — the test matrix
    ``omega`` (min(N, G) x l, l = min(k + p, N, G)) is drawn here, ``np.random.default_rng(seed).standard_normal``, unless given;
    the library itself holds no generator.  Returns ``d`` (k), ``u`` (N x k), ``v`` (G x k), ``cells`` = ``u * d`` (what the
    library computes; ``u`` is that divided by ``d``, zero where ``d`` is), ``centre`` (the gene means, or None).  Every
    component is signed so that the entry of largest magnitude of its ``v`` column is positive."""
    from . import _pca_lib

    M, colptr, rowidx, x = _csc_parts(A_csc_genes_x_cells)
    G, N = M.shape
    k, n = int(k), min(G, N)
    if omega is None:
        l = min(k + int(p), n)
        omega = np.random.default_rng(seed).standard_normal((n, l))
    omega = np.asfortranarray(omega, dtype=np.float64)
    if omega.ndim != 2 or omega.shape[0] != n:
        raise ValueError(f"omega must have min(N, G) = {n} rows")
    l = omega.shape[1]
    d = np.zeros(max(k, 1), dtype=np.float64)
    cells = np.zeros((max(k, 1), N), dtype=np.float64)        # C-order (k, N) == column-major N x k
    genes = np.zeros((max(k, 1), G), dtype=np.float64)
    mu = np.zeros(G, dtype=np.float64) if centre else None
    ctx = ctx or default_context()
    is64 = 1 if colptr.dtype == np.int64 else 0
    check(_pca_lib.load().gficf_rsvd_host(ctx.handle, G, N, _np_ptr(colptr), is64, _np_ptr(rowidx), _np_ptr(x), 1 if centre else 0,
                                          _np_ptr(omega), k, l, int(q), _np_ptr(d), _np_ptr(cells), _np_ptr(genes), _np_ptr(mu)))
    cells, genes = cells.T, genes.T
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(d > 0, cells / d, 0.0)
    return {"d": d, "u": u, "v": genes, "cells": cells, "centre": mu}


# ------------------------------------------------------------------ exact truncated SVD (libgficf_svds.so)
SVDS_MAX_B = 32
SVDS_MAX_M = 128


def svds(A_csc_genes_x_cells, k: int, centre: bool = False, tol: float = 1e-10, block: int = 8, m: int | None = None,
         max_cycles: int = 1000, seed: int = 180582, start=None, ctx: Context | None = None) -> dict:
    """``RSpectra::svds(t(M), k)`` for the genes x cells matrix ``M`` (scipy CSC): the k largest singular triplets of the cells x
    genes matrix ``A = t(M)``, with ``centre`` of ``A`` minus its column means (never densified), to the accuracy of f64 and
    independent of any random sketch.  The contract is the method of include/gficf_svds.h — block Lanczos with full
    reorthogonalisation and thick restart on the short side, n = min(N, G) — not RSpectra's bits: ``block`` is the block width
    b (at most 32, and at most ``m``), ``m`` the basis capacity (default min(n, 128); k + 2 b <= m unless m = n), ``tol``
    RSpectra's default.  The start block (n x b) is drawn here, ``np.random.default_rng(seed).standard_normal``, unless given;
    the library holds no generator, and the converged result does not depend on it beyond rounding.

    Returns :func:`rsvd`'s keys (``d``, ``u``, ``v``, ``cells``, ``centre``) plus ``residuals`` (k values
    ``||C v - theta v|| / theta`` as the iteration estimates them), ``converged`` (how many of the k pairs met ``tol``),
    ``cycles``, ``products`` (applications of the operator, two sparse products each) and ``exhausted`` (the Krylov space
    filled the whole space or closed: the result is then exact whatever ``converged`` says).  ``converged < k`` without
    exhaustion gives a warning naming the count, as RSpectra does, never an exception.  An eigenvalue of multiplicity above
    b is returned at most b times."""
    from . import _svds_lib

    M, colptr, rowidx, x = _csc_parts(A_csc_genes_x_cells)
    G, N = M.shape
    k, n = int(k), min(G, N)
    m = min(n, SVDS_MAX_M) if m is None else int(m)
    if start is None:
        start = np.random.default_rng(seed).standard_normal((n, max(1, min(int(block), m))))
    start = np.asfortranarray(start, dtype=np.float64)
    if start.ndim != 2 or start.shape[0] != n:
        raise ValueError(f"start must have min(N, G) = {n} rows")
    b = start.shape[1]
    kk = max(k, 1)
    d = np.zeros(kk, dtype=np.float64)
    cells = np.zeros((kk, N), dtype=np.float64)               # C-order (k, N) == column-major N x k
    genes = np.zeros((kk, G), dtype=np.float64)
    resid = np.zeros(kk, dtype=np.float64)
    info = np.zeros(4, dtype=np.int64)
    mu = np.zeros(G, dtype=np.float64) if centre else None
    ctx = ctx or default_context()
    is64 = 1 if colptr.dtype == np.int64 else 0
    check(_svds_lib.load().gficf_svds_host(ctx.handle, G, N, _np_ptr(colptr), is64, _np_ptr(rowidx), _np_ptr(x), 1 if centre else 0,
                                           _np_ptr(start), k, b, m, float(tol), int(max_cycles), _np_ptr(d), _np_ptr(cells), _np_ptr(genes),
                                           _np_ptr(mu), _np_ptr(resid), _np_ptr(info)))
    cells, genes = cells.T, genes.T
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(d > 0, cells / d, 0.0)
    converged, exhausted = int(info[2]), bool(info[3])
    if converged < k and not exhausted:
        warnings.warn(f"svds: only {converged} of the {k} singular values converged to tol = {tol:g} in {int(info[0])} cycles; "
                      "raise max_cycles or m, or see residuals", stacklevel=2)
    return {"d": d, "u": u, "v": genes, "cells": cells, "centre": mu, "residuals": resid, "converged": converged,
            "cycles": int(info[0]), "products": int(info[1]), "exhausted": exhausted}


# ------------------------------------------------------------------ NMF (libgficf_nmf.so)
NMF_MAX_K = 128
_NMF_OPS: dict = {}


def _nmf_ops(device: int = 0):
    """The stage object the NMF mirrors enqueue on (one per device, made at the first call)."""
    if device not in _NMF_OPS:
        _NMF_OPS[device] = HipOps(device)
    return _NMF_OPS[device]


def _nmf_pad(X, k: int, name: str, rows=None) -> np.ndarray:
    """``X`` (rows x k) as the library holds it: row-major float64 with the pitch ``_nmf_lib.ld(k)``, the padding zero."""
    from . import _nmf_lib

    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[1] != k or (rows is not None and X.shape[0] != rows):
        raise ValueError(f"{name} must be {'a matrix' if rows is None else rows} x {k}, not {X.shape}")
    out = np.zeros((X.shape[0], _nmf_lib.ld(k)), dtype=np.float64)
    out[:, :k] = X
    return out


def _nmf_limits(cd_tol, cd_maxit, ridge=0.0):
    if not (cd_tol >= 0 and ridge >= 0) or int(cd_maxit) < 0:
        raise ValueError("cd_tol, cd_maxit and ridge may not be negative")


def _nmf_matrix(A, name="A"):
    M, colptr, rowidx, x = _csc_parts(A)
    if len(x) and not (x.min() >= 0):
        raise ValueError(f"{name} holds a negative (or NaN) entry: the factorisation is of non-negative data")
    return M, colptr, rowidx, x


def _nmf_k(k, n: int) -> int:
    k = int(k)
    if not 1 <= k <= min(NMF_MAX_K, n):
        raise ValueError(f"k = {k}: 1 <= k <= min({NMF_MAX_K}, G, N) = {min(NMF_MAX_K, n)} is required")
    return k


class _NmfState:
    """The device tensors of one sparse matrix (n_in rows, n_out columns) and a workspace for k factors."""

    def __init__(self, A, k: int, device: int = 0):
        self.ops = _nmf_ops(device)
        tc = self.ops.torch
        self.tc, self.dev, self.k = tc, tc.device("cuda", device), int(k)
        M, colptr, rowidx, x = _nmf_matrix(A)
        self.n_in, self.n_out = M.shape
        self.colptr, self.rowidx, self.x = self.up(colptr.astype(np.int64)), self.up(rowidx), self.up(x)
        self.ws = tc.zeros(self.ops.nmf_workspace_bytes(self.n_in, self.n_out, len(x), self.k), dtype=tc.uint8, device=self.dev)

    def up(self, a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        if a.size == 0:
            a = np.zeros(1, dtype=a.dtype)
        return self.tc.from_numpy(a if a.flags.writeable else a.copy()).to(self.dev)

    def zeros(self, *shape, dtype=None):
        return self.tc.zeros(shape, dtype=dtype or self.tc.float64, device=self.dev)


def nnls(S, B, H0=None, cd_tol: float = 1e-8, cd_maxit: int = 100, ret_sweeps: bool = False, device: int = 0):
    """The batched non-negative least-squares solve of include/gficf_nmf.h: for every row ``b`` of ``B`` (M x k) the ``h >= 0``
    that minimises ``h'S h / 2 - b'h`` (``S``: k x k), by cyclic coordinate descent in a fixed order, started from ``H0``
    (M x k, non-negative) or from zero.  Returns ``H`` (M x k), with ``ret_sweeps`` also the sweeps every row took (int32)."""
    from . import _nmf_lib

    S = np.ascontiguousarray(S, dtype=np.float64)
    if S.ndim != 2 or S.shape[0] != S.shape[1] or not 1 <= S.shape[0] <= NMF_MAX_K:
        raise ValueError(f"S must be k x k with 1 <= k <= {NMF_MAX_K}")
    k = S.shape[0]
    _nmf_limits(cd_tol, cd_maxit)
    Bp = _nmf_pad(B, k, "B")
    M = Bp.shape[0]
    if M < 1:
        raise ValueError("B must have a row")
    H0p = None if H0 is None else _nmf_pad(H0, k, "H0", rows=M)
    if H0p is not None and not (H0p.min() >= 0):
        raise ValueError("H0 holds a negative (or NaN) entry")
    ops = _nmf_ops(device)
    tc, dev = ops.torch, ops.torch.device("cuda", device)
    H = tc.zeros((M, _nmf_lib.ld(k)), dtype=tc.float64, device=dev)
    sweeps = tc.zeros(M, dtype=tc.int32, device=dev)
    ws = tc.zeros(_nmf_lib.NNLS_WS_BYTES, dtype=tc.uint8, device=dev)
    ops.nnls(k, tc.from_numpy(S).to(dev), tc.from_numpy(Bp).to(dev), None if H0p is None else tc.from_numpy(H0p).to(dev), cd_tol, cd_maxit, H, sweeps, ws)
    ops.nmf_sync(ws)
    H = H.cpu().numpy()[:, :k].copy()
    return (H, sweeps.cpu().numpy()) if ret_sweeps else H


def nmf_half(A, X, Y=None, d=None, l1: float = 0.0, ridge: float = 1e-15, cd_tol: float = 1e-8, cd_maxit: int = 100, device: int = 0) -> dict:
    """One half-step of :func:`nmf` alone (steps 1 - 3 of include/gficf_nmf.h) on the sparse ``A`` (n_in x n_out): from the factor
    ``X`` (n_in x k) to the normalised factor ``y`` (n_out x k) and the scaling ``d``.  With ``Y`` and ``d`` (the previous
    factor and scaling) the solve starts from their product.  Also returned: ``S`` (k x k) and ``B`` (n_out x k) as the device
    formed them, ``sweeps`` per row, ``dead`` factors and ``capped`` rows."""
    from . import _nmf_lib

    X = np.asarray(X, dtype=np.float64)
    k = X.shape[1] if X.ndim == 2 else 0
    if not 1 <= k <= NMF_MAX_K:
        raise ValueError(f"X must be n_in x k with 1 <= k <= {NMF_MAX_K}")
    _nmf_limits(cd_tol, cd_maxit, ridge)
    s = _NmfState(A, k, device)
    tc, ldk, lpk = s.tc, _nmf_lib.ld(k), _nmf_lib.lp(k)
    Xd = s.up(_nmf_pad(X, k, "X", rows=s.n_in))
    warm = Y is not None
    if warm and d is None:
        raise ValueError("a warm start needs both Y and d")
    Yd = s.up(_nmf_pad(Y, k, "Y", rows=s.n_out)) if warm else s.zeros(s.n_out, ldk)
    dd = s.up(np.ascontiguousarray(d, dtype=np.float64).reshape(k)) if warm else s.zeros(k)
    S, B = s.zeros(lpk, lpk), s.zeros(s.n_out, ldk)
    sweeps, counts = s.zeros(s.n_out, dtype=tc.int32), s.zeros(2, dtype=tc.int64)
    s.ops.nmf_half(s.n_in, s.n_out, s.colptr, s.rowidx, s.x, len(_csc_parts(A)[3]), k, Xd, Yd, dd, warm, l1, ridge, cd_tol, cd_maxit, s.ws, S=S, B=B,
                   sweeps=sweeps, counts=counts)
    s.ops.nmf_sync(s.ws)
    counts = counts.cpu().numpy()
    return {"y": Yd.cpu().numpy()[:, :k].copy(), "d": dd.cpu().numpy(), "S": S.cpu().numpy()[:k, :k].copy(), "B": B.cpu().numpy()[:, :k].copy(),
            "sweeps": sweeps.cpu().numpy(), "dead": int(counts[0]), "capped": int(counts[1])}


def nmf_loss(A, w, d, h, device: int = 0, ret_terms: bool = False):
    """``||A - w diag(d) h||_F^2`` for the sparse ``A`` (G x N), ``w`` (G x k), ``d`` (k) and ``h`` (k x N), without densifying
    (include/gficf_nmf.h): ``||A||^2`` minus twice the cross term plus the quadratic term, which cancel once the fit is good,
    so its last digits mean nothing then.  ``ret_terms``: the four numbers ``(loss, ||A||^2, cross, quad)``."""
    w, h = np.asarray(w, dtype=np.float64), np.asarray(h, dtype=np.float64)
    k = w.shape[1] if w.ndim == 2 else 0
    if not 1 <= k <= NMF_MAX_K:
        raise ValueError(f"w must be G x k with 1 <= k <= {NMF_MAX_K}")
    s = _NmfState(A, k, device)
    if h.ndim != 2 or h.shape != (k, s.n_out):
        raise ValueError(f"h must be k x N = {k} x {s.n_out}, not {h.shape}")
    out = s.zeros(4)
    s.ops.nmf_loss(s.n_in, s.n_out, s.colptr, s.rowidx, s.x, len(_csc_parts(A)[3]), k, s.up(_nmf_pad(w, k, "w", rows=s.n_in)),
                   s.up(np.ascontiguousarray(d, dtype=np.float64).reshape(k)), s.up(_nmf_pad(h.T, k, "h")), out, s.ws)
    s.ops.nmf_sync(s.ws)
    out = out.cpu().numpy()
    return tuple(out) if ret_terms else float(out[0])


def nmf(A, k: int, seed: int = 180582, W0=None, tol: float = 1e-4, maxit: int = 100, L1=(0.0, 0.0), cd_tol: float = 1e-8, cd_maxit: int = 100,
        ridge: float = 1e-15, track_loss: bool = False, ctx: Context | None = None) -> dict:
    """Non-negative matrix factorisation ``A ~ w diag(d) h`` of the genes x cells matrix ``A`` (scipy CSC, non-negative) by
    alternating non-negative least squares on the device.  The contract is the method of include/gficf_nmf.h, not RcppML's or
    scikit-learn's bits: the start ``W0`` (G x k, non-negative) is drawn here, ``np.random.default_rng(seed).random((G, k))``,
    unless given (the library holds no generator); every solve is cyclic coordinate descent in one fixed order, stopped by a
    maximum (``cd_tol``, ``cd_maxit``); the iteration stops when ``1 - cor(w, w_previous) < tol`` or after ``maxit``
    iterations; ``L1 = (L1_w, L1_h)`` is subtracted from the right-hand sides; no masking, no symmetric shortcut.

    Returns ``w`` (G x k, columns sum to 1), ``d`` (k), ``h`` (k x N, rows sum to 1), ``cells`` = ``(diag(d) h)'`` (N x k, so that
    ``A ~ w cells'``, as ``runLSA`` has ``cells = u diag(d)``), ``iterations``, ``delta`` (one per iteration), ``converged``
    (``tol`` stopped it), ``loss`` (one per iteration with ``track_loss``, else None), ``dead`` (factors whose scaling fell to
    zero: they stay zero, never NaN) and ``capped_rows`` (rows of the last iteration whose solve ended at ``cd_maxit``).  A run
    that reaches ``maxit`` warns and names the last ``delta``; the same input gives the same bits on every call."""
    from . import _nmf_lib

    M, colptr, rowidx, x = _nmf_matrix(A)
    G, N = M.shape
    k = _nmf_k(k, min(G, N))
    L1 = tuple(float(v) for v in np.broadcast_to(np.asarray(L1, dtype=np.float64), (2,)))
    _nmf_limits(cd_tol, cd_maxit, ridge)
    if not (tol >= 0 and L1[0] >= 0 and L1[1] >= 0) or int(maxit) < 0:
        raise ValueError("tol, maxit and L1 may not be negative")
    if W0 is None:
        W0 = np.random.default_rng(seed).random((G, k))
    W0 = np.ascontiguousarray(W0, dtype=np.float64)
    if W0.shape != (G, k):
        raise ValueError(f"W0 must be G x k = {G} x {k}, not {W0.shape}")
    if not (W0.min() >= 0):
        raise ValueError("W0 holds a negative (or NaN) entry")
    maxit = int(maxit)
    w, d, h = np.zeros((G, k)), np.zeros(k), np.zeros((N, k))
    delta, loss, info = np.full(max(maxit, 1), np.nan), np.full(max(maxit, 1), np.nan), np.zeros(4, dtype=np.int64)
    ctx = ctx or default_context()
    is64 = 1 if colptr.dtype == np.int64 else 0
    check(_nmf_lib.load().gficf_nmf_host(ctx.handle, G, N, _np_ptr(colptr), is64, _np_ptr(rowidx), _np_ptr(x), k, _np_ptr(W0), float(tol), maxit,
                                         L1[0], L1[1], float(ridge), float(cd_tol), int(cd_maxit), 1 if track_loss else 0, _np_ptr(w), _np_ptr(d),
                                         _np_ptr(h), _np_ptr(delta), _np_ptr(loss), _np_ptr(info)))
    it, converged = int(info[0]), bool(info[1])
    if not converged and maxit > 0:
        warnings.warn(f"nmf: stopped after maxit = {maxit} iterations with delta = {delta[it - 1]:.3g} >= tol = {tol:g}; raise maxit or tol",
                      stacklevel=2)
    return {"w": w, "d": d, "h": np.ascontiguousarray(h.T), "cells": h * d, "iterations": it, "delta": delta[:it], "converged": converged,
            "loss": loss[:it] if track_loss else None, "dead": int(info[2]), "capped_rows": int(info[3]), "tol": float(tol), "seed": int(seed)}


def _pca_new_rows(data: dict, gficf_new, ctx):
    """The rows of ``gficf_new`` that ``data["pca"]`` decomposed (``gene_rows``), scaled by the stored ``gsf`` with ``rescale``."""
    if data["pca"].get("gene_rows") is None:
        return gficf_new
    od = data["pca"]["odgenes"]
    G_all = len(od["gsf"])
    if gficf_new.shape[0] != G_all:
        raise ValueError("gficf_new must have one row per row of data['gficf'] (data['pca']['odgenes'])")
    rows = np.asarray(data["pca"]["gene_rows"], dtype=np.int64)
    scale = np.ascontiguousarray(od["gsf"], dtype=np.float64) if data["pca"].get("rescale") else None
    every = len(rows) == G_all
    if scale is not None or not every:
        gficf_new = select_scale_rows(gficf_new, None if every else rows, scale, ctx)
    return gficf_new


def nmf_project(data_or_w, gficf_new, ridge=None, cd_tol=None, cd_maxit=None, ret_sweeps: bool = False, ctx: Context | None = None):
    """New cells against a trained NMF: ``data_or_w`` is the ``data`` of :func:`runNMF` or a ``w`` (G x k), ``gficf_new`` the
    genes x new-cells GF-ICF matrix over the same genes.  Every new cell ``a`` gets the ``c >= 0`` that minimises
    ``||a - w c||`` (``S = w'w + ridge``, ``B = gficf_new' w``, :func:`nnls` from zero): n_new x k, in the units of the
    training ``cells``.  The limits default to those of the training run (``data["pca"]["nmf"]``) or of :func:`nmf`."""
    from . import _nmf_lib

    kw = {"ridge": 1e-15, "cd_tol": 1e-8, "cd_maxit": 100}
    if isinstance(data_or_w, dict):
        pca = data_or_w.get("pca")
        if pca is None or pca.get("type") != "NMF":
            raise ValueError("First run runNMF")
        gficf_new = _pca_new_rows(data_or_w, gficf_new, ctx)
        w = pca["genes"]
        kw.update({n: pca["nmf"][n] for n in kw if n in pca.get("nmf", {})})
    else:
        w = data_or_w
    kw.update({n: v for n, v in (("ridge", ridge), ("cd_tol", cd_tol), ("cd_maxit", cd_maxit)) if v is not None})
    _nmf_limits(kw["cd_tol"], kw["cd_maxit"], kw["ridge"])
    w = np.ascontiguousarray(w, dtype=np.float64)
    M, colptr, rowidx, x = _nmf_matrix(gficf_new, "gficf_new")
    G, n_new = M.shape
    if w.ndim != 2 or w.shape[0] != G or not 1 <= w.shape[1] <= NMF_MAX_K:
        raise ValueError("gficf_new must have one row per row of w (data['pca']['genes']), and w at most 128 columns")
    k = w.shape[1]
    h, sweeps = np.zeros((n_new, k)), np.zeros(n_new, dtype=np.int32)
    ctx = ctx or default_context()
    is64 = 1 if colptr.dtype == np.int64 else 0
    check(_nmf_lib.load().gficf_nmf_project_host(ctx.handle, G, n_new, _np_ptr(colptr), is64, _np_ptr(rowidx), _np_ptr(x), k, _np_ptr(w),
                                                 float(kw["ridge"]), float(kw["cd_tol"]), int(kw["cd_maxit"]), _np_ptr(h), _np_ptr(sweeps)))
    return (h, sweeps) if ret_sweeps else h


def runNMF(data: dict, dim=None, seed: int = 180582, use_odgenes=False, n_odgenes=None, var_scale=False, ctx: Context | None = None,
           **nmf_kw) -> dict:
    """Non-negative matrix factorisation of ``data["gficf"]`` (:func:`nmf`; ``nmf_kw``: its ``tol``, ``maxit``, ``L1``, ``cd_tol``,
    ``cd_maxit``, ``ridge``, ``track_loss``, ``W0``) where :func:`runPCA` / :func:`runLSA` take a signed SVD: parts-based,
    non-negative gene programmes.  The reference has no such step; it sits where people put it, between ``gficf()`` and
    ``clustcells()``.  Gene selection is :func:`runPCA`'s (``use_odgenes="cr"`` / ``var_scale="cr"``; ``True`` is refused as
    there).  ``data["pca"]`` becomes ``{"cells": N x dim = (diag(d) h)', "genes": w (G x dim), "d", "h", "type": "NMF",
    "centre": False, "rescale", "mean": None, "nmf": {iterations, delta, converged, loss, dead, ...}}`` plus ``"odgenes"`` /
    ``"gene_rows"`` where used, so ``clustcells``, ``runReduction``, ``runTsne`` and ``runHarmony`` work on it unchanged, and
    :func:`pca_project` (``embedNewCells``, ``classify_cells(method="PCA")``) places new cells by :func:`nmf_project`."""
    if use_odgenes and data.get("rawCounts") is None:
        raise ValueError(_RAW_ABSENT)
    dim = _pca_dim(data, dim)
    _pca_unsupported(var_scale, use_odgenes, True)
    M, extra = _pca_matrix(data, var_scale, use_odgenes, n_odgenes, False, ctx)
    r = nmf(M, dim, seed=seed, ctx=ctx, **nmf_kw)
    how = {n: r[n] for n in ("iterations", "delta", "converged", "loss", "dead", "capped_rows", "tol", "seed")}
    how.update({"ridge": float(nmf_kw.get("ridge", 1e-15)), "cd_tol": float(nmf_kw.get("cd_tol", 1e-8)), "cd_maxit": int(nmf_kw.get("cd_maxit", 100))})
    data["pca"] = {"cells": r["cells"], "genes": r["w"], "d": r["d"], "h": r["h"], "type": "NMF", "centre": False, "rescale": bool(var_scale),
                   "mean": None, "nmf": how}
    data["pca"].update(extra)
    return data


# ------------------------------------------------------------------ overdispersed genes (libgficf_od.so)
_OD_COLUMNS = ("v", "fit", "res", "lp", "lpa", "qv", "gsf")
_RAW_ABSENT = "Raw Counts absent! Please run gficf normalization with storeRaw = T"


def _od_params(gam_k, sp, basis):
    from . import _od_lib

    if basis == "tp":
        raise NotImplementedError('basis="tp" is mgcv\'s thin-plate regression spline (an eigen-truncation on a random subsample of knots), '
                                  'which is not provided: pass basis="cr", the cubic regression spline (include/gficf_od.h)')
    if basis != "cr":
        raise ValueError('basis must be "cr"')
    gam_k = int(gam_k)
    if gam_k == 2 or gam_k > _od_lib.K_MAX:
        raise ValueError(f"gam_k must be below 2 (the straight line) or 3 to {_od_lib.K_MAX} (the knots of the spline)")
    sp = -1.0 if sp is None else float(sp)
    if not sp >= 0 and sp != -1.0:
        raise ValueError("sp must be None (the GCV search) or a smoothing parameter >= 0")
    return gam_k, sp


def _od_outputs(G: int) -> dict:
    from . import _od_lib

    o = {k: np.full(G, np.nan, dtype=np.float64) for k in _OD_COLUMNS}
    o["valid"] = np.zeros(G, dtype=np.int32)
    o["info"] = np.full(len(_od_lib.INFO), np.nan, dtype=np.float64)
    return o


def _od_result(o: dict, m, var, nobs) -> dict:
    from . import _od_lib

    info = dict(zip(_od_lib.INFO, o["info"]))
    kk = int(info["basis"])
    r = {"m": m, "var": var, "nobs": nobs, "valid": o["valid"] != 0}
    r.update({k: o[k] for k in _OD_COLUMNS})
    r.update({"n": int(info["n"]), "u": int(info["u"]), "basis": kk, "knots": o["info"][8:8 + kk].copy(), "lambda": float(info["lambda"]),
              "gcv": float(info["gcv"]), "edf": float(info["edf"]), "vbar": float(info["vbar"]), "rss": float(info["rss"])})
    return r


def over_dispersed_from_moments(m, var, nobs, N: int, gam_k: int = 5, min_gene_cells: int = 0, max_adjusted_variance: float = 1e3,
                                min_adjusted_variance: float = 1e-3, basis: str = "cr", sp=None, ctx: Context | None = None) -> dict:
    """Steps 1 - 6 of :func:`findOverDispersed` (include/gficf_od.h) from the genes' ICF weight ``m``, the variance ``var`` and
    the non-zero count ``nobs`` of their raw counts over ``N`` cells: ``v = log(var)``, ``valid``, the spline ``fit`` (NaN at an
    invalid gene), ``res``, ``lp``, ``lpa``, ``qv``, ``gsf`` per gene, and the fit's ``n``, ``u``, ``basis`` (the columns used:
    ``gam_k``, or 2 for the straight line, 1 for the mean), ``knots``, ``lambda``, ``gcv``, ``edf``, ``vbar``, ``rss``."""
    from . import _od_lib

    gam_k, sp = _od_params(gam_k, sp, basis)
    m, var = _hvg_vectors(m, var)
    nobs = np.ascontiguousarray(nobs, dtype=np.int32)
    if nobs.shape != m.shape:
        raise ValueError("m, var and nobs must be vectors of one length")
    if int(N) < 2:
        raise ValueError("the variance of a gene needs at least 2 cells")
    o = _od_outputs(len(m))
    ctx = ctx or default_context()
    check(_od_lib.load().gficf_od_from_moments_host(ctx.handle, len(m), int(N), _np_ptr(m), _np_ptr(var), _np_ptr(nobs), gam_k, int(min_gene_cells),
                                                    float(min_adjusted_variance), float(max_adjusted_variance), sp, _np_ptr(o["v"]), _np_ptr(o["valid"]),
                                                    _np_ptr(o["fit"]), _np_ptr(o["res"]), _np_ptr(o["lp"]), _np_ptr(o["lpa"]), _np_ptr(o["qv"]),
                                                    _np_ptr(o["gsf"]), _np_ptr(o["info"])))
    return _od_result(o, m, var, nobs)


def findOverDispersed(data: dict, gam_k: int = 5, alpha: float = .05, use_unadjusted_pvals: bool = False, max_adjusted_variance: float = 1e3,
                      min_adjusted_variance: float = 1e-3, verbose: bool = True, min_gene_cells: int = 0, basis: str = "cr", sp=None,
                      ret_stages: bool = False, ctx: Context | None = None):
    """``findOverDispersed(data, gam.k, alpha, ...)`` of the reference (R/dimensinalityReduction.R:235-291, after pagoda2) on
    the device, under the contract of include/gficf_od.h: every gene's log variance (of ``data["rawCounts"]``) regressed on its
    ICF weight ``data["w"]`` with a penalised spline of ``gam_k`` knots, the F-test log p-value ``lp`` of its residual, its BH
    adjustment in log space ``lpa``, the chi-square adjusted variance ``qv`` and the gene scale factor ``gsf``.  STATED
    DIFFERENCE: the spline is mgcv's cubic regression spline (``basis="cr"``, ``s(m, k, bs = "cr")`` with GCV), not its default
    thin-plate basis (``basis="tp"`` raises); ``sp`` fixes the smoothing parameter.  Returns a ``pandas.DataFrame`` with the
    columns ``m, v, nobs, res, lp, lpa, qv, gsf``, one row per row of ``data["gficf"]``.  ``ret_stages=True``: a dictionary with
    that ``table`` and ``fit, valid, knots, lambda, gcv, edf, n, u, basis`` and ``ods``, the rows below ``log(alpha)`` (of ``lpa``,
    or of ``lp`` with ``use_unadjusted_pvals``).  ``plot`` is not provided."""
    import pandas as pd

    from . import _od_lib

    gam_k, sp = _od_params(gam_k, sp, basis)
    if data.get("rawCounts") is None:
        raise ValueError(_RAW_ABSENT)
    tsmessage("calculating variance fit ...", verbose=verbose)
    M, colptr, rowidx, x = _csc_parts(data["rawCounts"])
    G, N = M.shape
    m = np.ascontiguousarray(data["w"], dtype=np.float64)
    if m.shape != (G,) or data["gficf"].shape[0] != G:
        raise ValueError("data['w'] and data['gficf'] must hold one entry per row of data['rawCounts']")
    if N < 2:
        raise ValueError("the variance of a gene needs at least 2 cells")
    o = _od_outputs(G)
    var, nobs = np.zeros(G, dtype=np.float64), np.zeros(G, dtype=np.int32)
    ctx = ctx or default_context()
    check(_od_lib.load().gficf_od_host(ctx.handle, G, N, _np_ptr(colptr), 1 if colptr.dtype == np.int64 else 0, _np_ptr(rowidx), _np_ptr(x), _np_ptr(m),
                                       gam_k, int(min_gene_cells), float(min_adjusted_variance), float(max_adjusted_variance), sp, _np_ptr(var),
                                       _np_ptr(nobs), _np_ptr(o["v"]), _np_ptr(o["valid"]), _np_ptr(o["fit"]), _np_ptr(o["res"]), _np_ptr(o["lp"]),
                                       _np_ptr(o["lpa"]), _np_ptr(o["qv"]), _np_ptr(o["gsf"]), _np_ptr(o["info"])))
    r = _od_result(o, m, var, nobs)
    tsmessage(" using lm " if r["basis"] <= 2 else " using gam ", verbose=verbose)
    ods = np.flatnonzero((r["lp"] if use_unadjusted_pvals else r["lpa"]) < np.log(alpha))
    tsmessage(f"{len(ods)}overdispersed genes ...{len(ods)}", verbose=verbose)
    tsmessage("done.\n", verbose=verbose)
    table = pd.DataFrame({k: r[k] for k in ("m", "v", "nobs", "res", "lp", "lpa", "qv", "gsf")})
    if not ret_stages:
        return table
    out = {k: r[k] for k in ("fit", "valid", "var", "knots", "lambda", "gcv", "edf", "n", "u", "basis", "vbar", "rss")}
    out.update({"table": table, "ods": ods})
    return out


def _od_dev(device: int):
    ops = _umap_hip(device)
    tc = ops.torch
    dev = tc.device("cuda", device)
    return ops, tc, dev, (lambda v, dt=np.float64: tc.from_numpy(np.array(v, dtype=dt, order="C")).to(dev))


def log_pf(res, df, device: int = 0) -> np.ndarray:
    """``pf(exp(res), df, df, lower.tail = FALSE, log.p = TRUE)`` in log space (step 3 of include/gficf_od.h): the log of the
    regularised incomplete beta ``I_z(df / 2, df / 2)`` at ``z = 1 / (1 + exp(res))``, far into either tail.  ``res = -Inf``
    gives 0, ``df = 0`` NaN."""
    res = np.ascontiguousarray(res, dtype=np.float64)
    a = np.array(np.broadcast_to(np.asarray(df, dtype=np.float64) / 2.0, res.shape), dtype=np.float64, order="C")
    if res.size == 0:
        return np.zeros(res.shape)
    ops, tc, dev, t = _od_dev(device)
    ws = tc.zeros(ops.od_workspace_bytes(res.size), dtype=tc.uint8, device=dev)
    out = tc.empty(res.size, dtype=tc.float64, device=dev)
    ops.od_logpf(t(res.ravel()), t(a.ravel()), ws, out)
    ops.od_sync(ws)
    return out.cpu().numpy().reshape(res.shape)


def log_qchisq(lp, df: float, device: int = 0) -> np.ndarray:
    """``qchisq(lp, df, lower.tail = FALSE, log.p = TRUE)`` (step 5 of include/gficf_od.h): the ``x`` whose upper chi-square
    tail has the log probability ``lp``, by Newton in log space.  ``lp = 0`` gives 0, ``lp = -Inf`` Inf; ``lp > 0`` or NaN, or
    ``df <= 0``, NaN.  A value whose iteration hits its cap raises."""
    lp = np.ascontiguousarray(lp, dtype=np.float64)
    if lp.size == 0:
        return np.zeros(lp.shape)
    ops, tc, dev, t = _od_dev(device)
    ws = tc.zeros(ops.od_workspace_bytes(lp.size), dtype=tc.uint8, device=dev)
    out = tc.empty(lp.size, dtype=tc.float64, device=dev)
    ops.od_logqchisq(t(lp.ravel()), float(df), ws, out)
    ops.od_sync(ws)
    return out.cpu().numpy().reshape(lp.shape)


def bh_adjust_log(lp, device: int = 0) -> np.ndarray:
    """``bh.adjust(lp, log = TRUE)`` of the reference (R/dimensinalityReduction.R:294-308), literally, on the device: over the
    non-NaN ``lp`` in ascending order (ties by position) ``lp + log(n / rank)``, the running minimum from the end; NaN stays."""
    lp = np.ascontiguousarray(lp, dtype=np.float64)
    if lp.ndim != 1 or len(lp) < 1:
        raise ValueError("lp must be a vector")
    ops, tc, dev, t = _od_dev(device)
    ws = tc.zeros(ops.od_workspace_bytes(len(lp)), dtype=tc.uint8, device=dev)
    out = tc.empty(len(lp), dtype=tc.float64, device=dev)
    ops.od_bh_log(t(lp), ws, out)
    ops.od_sync(ws)
    return out.cpu().numpy()


def select_scale_rows(M, rows=None, scale=None, ctx: Context | None = None):
    """The rows ``rows`` of the genes x cells matrix ``M`` (scipy sparse), renumbered in ascending order, each multiplied by
    its entry of ``scale`` (one per row of ``M``; None: 1), as a scipy CSC matrix: ``x[, odgenes]`` and ``x@x * gsf`` of the
    reference's ``runPCA`` in one pass on the device.  An entry whose scale is 0 stays stored, as 0.  ``rows=None``: every row
    (only the values change).  Selecting no row is an error, not an empty decomposition."""
    import scipy.sparse as sp

    from . import _od_lib

    M, colptr, rowidx, x = _csc_parts(M)
    G, N = M.shape
    mask = None
    if rows is not None:
        rows = np.asarray(rows, dtype=np.int64).ravel()
        if len(rows) == 0:
            raise ValueError("select_scale_rows: no row is selected: there is nothing to decompose")
        if rows.min() < 0 or rows.max() >= G or len(np.unique(rows)) != len(rows):
            raise ValueError(f"rows must name distinct rows of M (0 .. {G - 1})")
        mask = np.zeros(G, dtype=np.int32)
        mask[rows] = 1
    if scale is not None:
        scale = np.ascontiguousarray(scale, dtype=np.float64)
        if scale.shape != (G,):
            raise ValueError("scale must hold one value per row of M")
    if G < 1:
        raise ValueError("M must hold at least one row")
    nnz = len(x)
    out_x = np.zeros(max(nnz, 1), dtype=np.float64)
    out_cp = np.zeros(N + 1, dtype=np.int64)
    out_row = np.zeros(max(nnz, 1), dtype=np.int32)
    nsel = np.zeros(1, dtype=np.int32)
    ctx = ctx or default_context()
    check(_od_lib.load().gficf_od_select_scale_host(ctx.handle, G, N, _np_ptr(colptr), 1 if colptr.dtype == np.int64 else 0, _np_ptr(rowidx), _np_ptr(x),
                                                    _np_ptr(mask), _np_ptr(scale), _np_ptr(out_cp), _np_ptr(out_row), _np_ptr(out_x), _np_ptr(nsel)))
    if mask is None:
        return sp.csc_matrix((out_x[:nnz], rowidx, colptr), shape=(G, N))
    n_out = int(out_cp[N])
    return sp.csc_matrix((out_x[:n_out], out_row[:n_out], out_cp.astype(colptr.dtype)), shape=(int(nsel[0]), N))


def odgenes_rows(overD, n_odgenes=None) -> np.ndarray:
    """The rows ``runPCA(use.odgenes = T, n.odgenes)`` of the reference decomposes (R/dimensinalityReduction.R:103-113), in
    ascending order: those with ``lpa < log(0.1)``; with ``n_odgenes`` at most that many, the first ``n_odgenes`` of them in row
    order (the reference's own quirk); with ``n_odgenes`` more than that many, the ``min(G, n_odgenes)`` rows of smallest ``lp``
    (ordered stably, NaN last).  ``overD``: the table of :func:`findOverDispersed`."""
    lp, lpa = np.asarray(overD["lp"], dtype=np.float64), np.asarray(overD["lpa"], dtype=np.float64)
    rows = np.flatnonzero(lpa < np.log(0.1))
    if n_odgenes is not None:
        n_odgenes = int(n_odgenes)
        if n_odgenes > len(rows):
            rows = np.argsort(lp, kind="stable")[:min(len(lp), n_odgenes)]
        else:
            rows = rows[:n_odgenes]
    return np.sort(rows).astype(np.int64)


def _pca_dim(data: dict, dim):
    if dim is None:
        if data.get("dimPCA") is None:
            raise ValueError("Specify the number of dims or run computePCADim first")
        return int(data["dimPCA"])
    data["dimPCA"] = int(dim)
    return int(dim)


def _pca_unsupported(var_scale, use_odgenes, randomized):
    for name, value in (("use_odgenes", use_odgenes), ("var_scale", var_scale)):
        if isinstance(value, str) and value != "cr":
            raise ValueError(f'{name} must be False or "cr"')
    if any(v and not isinstance(v, str) for v in (use_odgenes, var_scale)):
        raise NotImplementedError("use_odgenes / var_scale need findOverDispersed (the mgcv::gam fit of the reference), which is not "
                                  "provided on mgcv's default thin-plate basis: pass use_odgenes=\"cr\" / var_scale=\"cr\" for the same model "
                                  "on its cubic regression spline (include/gficf_od.h), or use_odgenes=False and var_scale=False")
    _pca_randomized(randomized)


def _pca_randomized(randomized):
    """``True`` (the randomized SVD, :func:`rsvd`) or ``"svds"`` (the exact one, :func:`svds`).  ``False`` stands for the
    reference's RSpectra::svds / prcomp, whose bits are not provided: the exact decomposition has its own spelling, as
    ``hvg="locfit"`` and ``var_scale="cr"`` have."""
    if isinstance(randomized, str):
        if randomized != "svds":
            raise ValueError('randomized must be True or "svds"')
        return "svds"
    if not randomized:
        raise NotImplementedError("randomized=False is the reference's full decomposition (RSpectra::svds / prcomp), which is not "
                                  'provided: pass randomized=True, or randomized="svds" for the exact truncated SVD of '
                                  "include/gficf_svds.h")
    return True


def _pca_decompose(M, k, randomized, seed, centre, ctx):
    """(the decomposition, what ``data["pca"]`` also stores about it): :func:`rsvd`, or :func:`svds` for ``randomized="svds"``."""
    if _pca_randomized(randomized) == "svds":
        r = svds(M, k, centre=centre, seed=seed, ctx=ctx)
        return r, {"svds": {"converged": r["converged"], "residuals": r["residuals"], "cycles": r["cycles"]}}
    return rsvd(M, k, seed=seed, centre=centre, ctx=ctx), {}


def _pca_matrix(data: dict, var_scale, use_odgenes, n_odgenes, plot_odgenes, ctx):
    """The matrix ``runPCA`` / ``runLSA`` decompose and what they store about it (R/dimensinalityReduction.R:103-122): with
    ``use_odgenes="cr"`` the overdispersed rows (:func:`odgenes_rows`), with ``var_scale="cr"`` every row times its ``gsf``."""
    if not use_odgenes and not var_scale:
        return data["gficf"], {}
    if plot_odgenes:
        warnings.warn("plot_odgenes=True (the reference's smoothScatter plots) is not provided: ignored", stacklevel=3)
    overD = findOverDispersed(data, alpha=0.1, verbose=False, ctx=ctx)
    G = data["gficf"].shape[0]
    rows = odgenes_rows(overD, n_odgenes) if use_odgenes else np.arange(G, dtype=np.int64)
    if use_odgenes:
        if len(rows) == 0:
            raise ValueError("use_odgenes: no gene is overdispersed (lpa < log(0.1)): there is nothing to decompose; pass n_odgenes")
        tsmessage("... using ", len(rows), " OD genes", verbose=True)
    scale = np.ascontiguousarray(overD["gsf"], dtype=np.float64) if var_scale else None
    M = select_scale_rows(data["gficf"], rows if use_odgenes else None, scale, ctx)
    return M, {"odgenes": overD, "gene_rows": rows}


def runPCA(data: dict, dim=None, var_scale=False, centre: bool = False, randomized: bool = True, seed: int = 180582,
           use_odgenes=False, n_odgenes=None, plot_odgenes: bool = False, ctx: Context | None = None) -> dict:
    """``runPCA(data, dim, var.scale, centre, randomized, seed, use.odgenes, n.odgenes, plot.odgenes)`` of the reference
    (R/dimensinalityReduction.R:85-133): ``rsvd::rpca(t(data$gficf), k = dim, center = centre, scale = F)`` on the device
    (:func:`rsvd`, relaxed contract).  ``data["pca"]`` becomes ``{"cells": N x dim (rpca's x), "genes": G x dim (its rotation),
    "centre": centre, "rescale": var_scale}`` plus ``"mean"``, the gene means that were subtracted (None without ``centre``; the
    reference's centring densifies and keeps nothing for later), and ``data["dimPCA"] = dim``.

    ``randomized="svds"`` runs the exact truncated SVD instead (:func:`svds`: no sketch, no dependence on a test matrix) and
    adds ``data["pca"]["svds"] = {"converged", "residuals", "cycles"}``; ``randomized=False``, the reference's spelling of
    RSpectra::svds / prcomp, is refused.

    ``use_odgenes="cr"`` decomposes only the overdispersed genes of :func:`findOverDispersed` (:func:`odgenes_rows`, in
    ascending row order: where the reference decomposes in ``order(lp)`` order the result is a permutation of the same
    columns), ``var_scale="cr"`` scales every gene by its ``gsf`` first; either alone or both (:func:`select_scale_rows`).
    ``data["pca"]`` then also holds ``"odgenes"`` (the table) and ``"gene_rows"`` (the rows of ``data["gficf"]`` decomposed,
    one per row of ``"genes"``), which :func:`pca_project` applies to new cells.  ``True`` stands for the reference's fit on
    mgcv's default thin-plate basis, which is not provided.  ``plot_odgenes`` is accepted and ignored, with a warning."""
    if use_odgenes and data.get("rawCounts") is None:
        raise ValueError(_RAW_ABSENT)
    dim = _pca_dim(data, dim)
    _pca_unsupported(var_scale, use_odgenes, randomized)
    M, extra = _pca_matrix(data, var_scale, use_odgenes, n_odgenes, plot_odgenes, ctx)
    r, how = _pca_decompose(M, dim, randomized, seed, bool(centre), ctx)
    data["pca"] = {"cells": r["cells"], "genes": r["v"], "centre": bool(centre), "rescale": bool(var_scale), "mean": r["centre"]}
    data["pca"].update(extra)
    data["pca"].update(how)
    return data


def runLSA(data: dict, dim=None, var_scale=False, centre: bool = False, randomized: bool = True, seed: int = 180582,
           use_odgenes=False, n_odgenes=None, plot_odgenes: bool = False, ctx: Context | None = None) -> dict:
    """``runLSA(...)`` of the reference (R/dimensinalityReduction.R:19-65): ``rsvd::rsvd(t(data$gficf), k = dim)``, then
    ``cells = u %*% diag(d)`` and ``genes = v``.  As in the reference ``centre`` is accepted and not used
    (``data$pca$centre <- F``, :59).  ``use_odgenes="cr"`` / ``var_scale="cr"`` / ``randomized="svds"``: as in :func:`runPCA`."""
    if use_odgenes and data.get("rawCounts") is None:
        raise ValueError(_RAW_ABSENT)
    dim = _pca_dim(data, dim)
    _pca_unsupported(var_scale, use_odgenes, randomized)
    M, extra = _pca_matrix(data, var_scale, use_odgenes, n_odgenes, plot_odgenes, ctx)
    r, how = _pca_decompose(M, dim, randomized, seed, False, ctx)
    data["pca"] = {"cells": r["cells"], "genes": r["v"], "centre": False, "rescale": bool(var_scale), "mean": None}
    data["pca"].update(extra)
    data["pca"].update(how)
    return data


def pca_dim_rule(d):
    """The elbow rule of ``computePCADim`` (reference R/dimensinalityReduction.R:219-225), literally: the shares
    ``d^2 / sum(d^2)`` over the values computed, their successive differences relative to the first one, the 1-based positions
    ``w`` where that ratio is below 0.1, and ``w[ix]`` for the first ``ix`` at which ``cumsum(diff(w) == 1)`` exceeds 1.
    Returns None where R would give NA."""
    d = np.asarray(d, dtype=np.float64)
    ev = d ** 2 / np.sum(d ** 2)
    df = np.diff(ev)
    if len(df) == 0:
        return None
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = df / df[0]
    w = np.flatnonzero(ratio < 0.1) + 1
    hit = np.flatnonzero(np.cumsum(np.diff(w) == 1) > 1)
    return int(w[hit[0]]) if len(hit) else None


def computePCADim(data: dict, randomized: bool = True, subsampling: bool = False, plot: bool = False, seed: int = 180582,
                  ctx: Context | None = None) -> dict:
    """``computePCADim(data, randomized, subsampling, plot)`` of the reference (R/dimensinalityReduction.R:206-230):
    ``rsvd(t(data$gficf), k = min(50, N))`` and the elbow rule (:func:`pca_dim_rule`) on its ``d``; ``data["dimPCA"]`` is set
    and the reference's line printed.  ``subsampling``: 5 % of the cells, drawn with numpy's generator from ``seed`` (the
    reference uses R's ``sample``).  ``randomized="svds"``: the rule on the exact values (:func:`svds`).  Raises where the
    reference would store NA."""
    _pca_randomized(randomized)
    M = data["gficf"]
    N = M.shape[1]
    if subsampling:
        pick = np.random.default_rng(seed).choice(N, size=int(round(N / 100 * 5)), replace=False)
        M = M[:, pick]
    d = _pca_decompose(M, min(50, M.shape[1]), randomized, seed, False, ctx)[0]["d"]
    if plot:
        try:
            import matplotlib.pyplot as plt

            plt.plot(np.arange(1, len(d) + 1), d ** 2 / np.sum(d ** 2), "o")
            plt.xlabel("components")
            plt.ylabel("explained.var")
        except ImportError:
            warnings.warn("computePCADim: plot=True needs matplotlib, which is not installed", stacklevel=2)
    dim = pca_dim_rule(d)
    if dim is None:
        raise ValueError("computePCADim: the elbow rule selects no dimension (the reference would store NA)")
    print("Number of estimated dimensions =", dim)
    data["dimPCA"] = dim
    return data


def pca_project(data: dict, gficf_new, ctx: Context | None = None) -> np.ndarray:
    """``x %*% data$pca$genes`` of ``embedNewCells`` (reference R/cellClassifier.R:54-64) for ``gficf_new``, the genes x
    new-cells GF-ICF matrix of :func:`gficf_with_weights` over the genes of ``data["pca"]["genes"]``: the new cells in the PCA
    space, n_new x dim.  After ``runPCA(centre=True)`` the training gene means are subtracted first (the reference's
    ``scaleMatrix`` is a stub that does nothing).  After ``use_odgenes="cr"`` / ``var_scale="cr"`` (``data["pca"]["gene_rows"]``)
    ``gficf_new`` has one row per row of ``data["gficf"]``: the rows decomposed are selected and, with ``rescale``, scaled by
    the stored ``gsf`` first (:func:`select_scale_rows`; reference R/cellClassifier.R:56-62).  After :func:`runNMF`
    (``data["pca"]["type"] == "NMF"``) the new cells are placed by the non-negative projection :func:`nmf_project` instead."""
    from . import _pca_lib

    if data.get("pca") is None:
        raise ValueError("First run runPCA or runLSA to reduce dimensionality")
    if data["pca"].get("type") == "NMF":
        return nmf_project(data, gficf_new, ctx=ctx)
    gficf_new = _pca_new_rows(data, gficf_new, ctx)
    genes = np.asfortranarray(data["pca"]["genes"], dtype=np.float64)
    M, colptr, rowidx, x = _csc_parts(gficf_new)
    G, n_new = M.shape
    if genes.ndim != 2 or genes.shape[0] != G:
        raise ValueError("gficf_new must have one row per row of data['pca']['genes']")
    k = genes.shape[1]
    mu = None
    if data["pca"].get("centre"):
        mu = np.ascontiguousarray(data["pca"]["mean"], dtype=np.float64)
    out = np.zeros((k, n_new), dtype=np.float64)              # C-order (k, n_new) == column-major n_new x k
    ctx = ctx or default_context()
    is64 = 1 if colptr.dtype == np.int64 else 0
    check(_pca_lib.load().gficf_pca_project_host(ctx.handle, G, n_new, _np_ptr(colptr), is64, _np_ptr(rowidx), _np_ptr(x), _np_ptr(genes), k,
                                                 _np_ptr(mu), _np_ptr(out)))
    return out.T


# ------------------------------------------------------------------ embedding (libgficf_umap.so)
REDUCTIONS = ("tumap", "umap")
_REDUCTION_KW = {"n_neighbors": 15, "metric": "euclidean", "n_epochs": None, "learning_rate": 1.0, "min_dist": 0.01, "spread": 1.0, "a": None,
                 "b": None, "negative_sample_rate": 5, "repulsion_strength": 1.0, "set_op_mix_ratio": 1.0, "local_connectivity": 1.0,
                 "init": "pca"}
_umap_ops: dict = {}


def _umap_hip(device: int = 0) -> "HipOps":
    """The device-resident stages behind the host-data building blocks (torch owns their device memory)."""
    if device not in _umap_ops:
        _umap_ops[device] = HipOps(device)
    return _umap_ops[device]


def find_ab_params(spread: float = 1.0, min_dist: float = 0.01):
    """The curve parameters ``a``, ``b`` of UMAP for ``spread`` and ``min_dist``, fitted on the host as umap-learn's
    ``find_ab_params`` does: least squares (``scipy.optimize.curve_fit``) of ``1 / (1 + a x^(2b))`` to the curve that is 1 for
    ``x < min_dist`` and ``exp(-(x - min_dist) / spread)`` beyond, on ``linspace(0, 3 spread, 300)``."""
    from scipy.optimize import curve_fit

    spread, min_dist = float(spread), float(min_dist)
    if not spread > 0 or not min_dist >= 0:
        raise ValueError("spread must be positive and min_dist non-negative")
    xv = np.linspace(0.0, 3.0 * spread, 300)
    yv = np.where(xv < min_dist, 1.0, np.exp(-(xv - min_dist) / spread))
    (a, b), _ = curve_fit(lambda x, a, b: 1.0 / (1.0 + a * x ** (2.0 * b)), xv, yv)
    return float(a), float(b)


def umap_init(init, pca_cells, N: int, seed: int) -> np.ndarray:
    """The initial coordinates of :func:`runReduction`, N x 2 float64.  ``"pca"``: the first two columns of ``pca_cells`` scaled
    to a largest magnitude of 10, plus normal noise of standard deviation 1e-4 from ``default_rng(seed)``; ``"random"``: uniform
    on [-10, 10) from the same generator; an N x 2 array is taken as it is.  ``"spectral"`` (uwot's default) needs the graph, not
    the cells: :func:`spectral_init` computes it, and :func:`umap` takes the string."""
    if isinstance(init, str):
        if init == "spectral":
            raise NotImplementedError("init='spectral' (uwot's default) is not wired into runReduction: call gficf_amd.umap(..., "
                                      "init='spectral') or pass init=gficf_amd.spectral_init(graph); init='normlaplacian', 'pca' (the "
                                      "default here), 'random' and an N x 2 array are taken")
        if init not in ("pca", "random"):
            raise ValueError("init must be 'pca', 'random' or an N x 2 array")
        rng = np.random.default_rng(seed)
        if init == "random":
            return rng.uniform(-10.0, 10.0, size=(N, 2))
        if pca_cells is None or np.ndim(pca_cells) != 2 or np.shape(pca_cells)[1] < 2:
            raise ValueError("init='pca' needs at least two PCA components")
        Y = np.array(np.asarray(pca_cells)[:, :2], dtype=np.float64)
        top = np.abs(Y).max()
        if top > 0:
            Y *= 10.0 / top
        return Y + rng.normal(0.0, 1e-4, size=(N, 2))
    Y = np.array(init, dtype=np.float64)
    if Y.shape != (N, 2):
        raise ValueError(f"init must be 'pca', 'random' or an N x 2 = {N} x 2 array")
    return Y


def fuzzy_simplicial_set(idx, dist, set_op_mix_ratio: float = 1.0, local_connectivity: float = 1.0, ret_memberships: bool = False,
                         device: int = 0):
    """UMAP's fuzzy graph from a neighbour table as :func:`find_nn` returns it (``idx`` N x k, 1-based, column 0 the nearest
    point; ``dist`` alike): the smoothed memberships and their symmetrisation (``gficf_umap_graph_device``, include/gficf_umap.h).
    Returns ``(P, sigma, rho)``: the N x N scipy CSR matrix (float32, columns ascending, ``P == P.T`` bit for bit) and the two
    float32 vectors; with ``ret_memberships`` also ``W``, the N x k float32 memberships before the symmetrisation."""
    import scipy.sparse as sp

    idx, dist = np.asarray(idx), np.asarray(dist)
    if idx.ndim != 2 or idx.shape != dist.shape:
        raise ValueError("idx and dist must be N x k matrices of the same shape")
    N, k = idx.shape
    ops = _umap_hip(device)
    tc, dev = ops.torch, f"cuda:{device}"
    d_idx = tc.from_numpy(np.ascontiguousarray(idx.T, dtype=np.int32)).to(dev)         # (k, N) C-order == column-major N x k
    d_dist = tc.from_numpy(np.ascontiguousarray(dist.T, dtype=np.float32)).to(dev)
    cap = 2 * N * k
    ws = tc.empty(max(ops.umap_graph_workspace_bytes(N, k), 1), dtype=tc.uint8, device=dev)
    rowptr = tc.empty(N + 1, dtype=tc.int64, device=dev)
    col = tc.empty(max(cap, 1), dtype=tc.int32, device=dev)
    val = tc.empty(max(cap, 1), dtype=tc.float32, device=dev)
    nnz = tc.zeros(1, dtype=tc.int64, device=dev)
    sigma = tc.empty(max(N, 1), dtype=tc.float32, device=dev)
    rho = tc.empty(max(N, 1), dtype=tc.float32, device=dev)
    w = tc.empty((max(k, 1), max(N, 1)), dtype=tc.float32, device=dev) if ret_memberships else None
    ops.umap_graph(d_idx, d_dist, N, k, ws, rowptr, col, val, nnz, set_op_mix_ratio, local_connectivity, sigma, rho, w)
    ops.umap_sync(ws)
    n = int(nnz.item())
    P = sp.csr_matrix((val[:n].cpu().numpy(), col[:n].cpu().numpy(), rowptr.cpu().numpy()), shape=(N, N))
    if ret_memberships:
        return P, sigma.cpu().numpy(), rho.cpu().numpy(), np.ascontiguousarray(w.cpu().numpy().T)
    return P, sigma.cpu().numpy(), rho.cpu().numpy()


def umap_layout(P, init, n_epochs: int, a: float = 1.0, b: float = 1.0, learning_rate: float = 1.0, negative_sample_rate: int = 5,
                repulsion_strength: float = 1.0, seed: int = 0, epoch_begin: int = 0, epoch_end=None, device: int = 0) -> np.ndarray:
    """Epochs ``[epoch_begin, epoch_end)`` of ``n_epochs`` of the UMAP layout over the symmetric graph ``P`` (scipy sparse,
    taken as CSR with sorted columns) from the coordinates ``init`` (N x 2): ``gficf_umap_layout_device``, the integer schedule
    and the owner-computes update of include/gficf_umap.h.  Returns the N x 2 float32 coordinates; running ``[0, a)`` and then
    ``[a, n)`` from its result gives the bits of ``[0, n)``."""
    csr = _square_csr(P)
    N = csr[0]
    Y = np.ascontiguousarray(init, dtype=np.float32)
    if Y.shape != (N, 2):
        raise ValueError(f"init must be an N x 2 = {N} x 2 array")
    epoch_end = int(n_epochs) if epoch_end is None else int(epoch_end)
    ops = _umap_hip(device)
    tc, dev = ops.torch, f"cuda:{device}"
    _, cap, rowptr, col, val = _dev_csr(ops, csr, device)
    d_Y = tc.from_numpy(Y).to(dev)
    ws = tc.empty(max(ops.umap_layout_workspace_bytes(N, cap), 1), dtype=tc.uint8, device=dev)
    ops.umap_layout(N, rowptr, col, val, cap, a, b, repulsion_strength, learning_rate, negative_sample_rate, n_epochs, epoch_begin, epoch_end, seed,
                    d_Y, ws)
    ops.umap_sync(ws)
    return d_Y.cpu().numpy()


def _square_csr(P, allow_arrays: bool = False):
    """``(N, indptr int64, indices int32, data float32)`` of the graph ``P``: a square scipy sparse matrix, taken as CSR with
    sorted columns; with ``allow_arrays`` also the three arrays themselves as ``(indptr, indices, data)``, which are handed to
    the library unchecked."""
    import scipy.sparse as sp

    if allow_arrays and isinstance(P, tuple):
        indptr, indices, data = P
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        return len(indptr) - 1, indptr, np.ascontiguousarray(indices, dtype=np.int32), np.ascontiguousarray(data, dtype=np.float32)
    P = sp.csr_matrix(P)
    if P.shape[0] != P.shape[1]:
        raise ValueError("P must be square")
    if not P.has_sorted_indices:
        P = P.sorted_indices()
    return P.shape[0], P.indptr.astype(np.int64), np.ascontiguousarray(P.indices, dtype=np.int32), np.ascontiguousarray(P.data, dtype=np.float32)


def _dev_csr(ops, csr, device):
    """What :func:`_square_csr` returned, on the device: ``(N, cap, rowptr, col, val)``; an empty graph gets 1-element
    placeholders, so every pointer handed to the library is valid."""
    tc, dev = ops.torch, f"cuda:{device}"
    N, indptr, indices, data = csr
    cap = int(len(indices))
    rowptr = tc.from_numpy(indptr).to(dev)
    col = tc.from_numpy(indices).to(dev) if cap else tc.empty(1, dtype=tc.int32, device=dev)
    val = tc.from_numpy(data).to(dev) if cap else tc.empty(1, dtype=tc.float32, device=dev)
    return N, cap, rowptr, col, val


def _spectral_csr(P):
    csr = _square_csr(P)
    if csr[0] < 1:
        raise ValueError("P has no vertices")
    return csr


def graph_components(P, ret_rounds: bool = False, device: int = 0):
    """The connected components of the graph ``P`` (scipy sparse, square; an entry (i, j) joins i and j whether or not (j, i) is
    stored): ``gficf_graph_components_device`` (include/gficf_spectral.h), hook and pointer-jump on the device.  Returns
    ``(labels, n)``: ``labels[i]`` (int32) is the smallest vertex id of i's component, ``n`` the number of components; with
    ``ret_rounds`` also the number of rounds it took."""
    csr = _spectral_csr(P)
    ops = _umap_hip(device)
    tc, dev = ops.torch, f"cuda:{device}"
    N, cap, rowptr, col, _ = _dev_csr(ops, csr, device)
    labels = tc.empty(N, dtype=tc.int32, device=dev)
    info = tc.zeros(2, dtype=tc.int64, device=dev)
    ws = tc.empty(max(ops.graph_components_workspace_bytes(N), 1), dtype=tc.uint8, device=dev)
    ops.graph_components(N, rowptr, col, cap, labels, info, ws)
    info = info.cpu().numpy()
    if ret_rounds:
        return labels.cpu().numpy(), int(info[0]), int(info[1])
    return labels.cpu().numpy(), int(info[0])


def _spectral_args(N: int, ndim, m, tol, max_restarts, start):
    """The checks of include/gficf_spectral.h that need no device (the library would say the same); the start block or None."""
    from . import _spectral_lib

    ndim, m, max_restarts = int(ndim), int(m), int(max_restarts)
    if not 1 <= ndim <= _spectral_lib.MAX_NDIM:
        raise ValueError(f"ndim = {ndim} outside [1, {_spectral_lib.MAX_NDIM}]")
    if N <= ndim:
        raise ValueError(f"N = {N} vertices for ndim = {ndim}: N must exceed ndim")
    if not 2 * ndim + 2 <= m <= _spectral_lib.MAX_M:
        raise ValueError(f"m = {m} outside [2 ndim + 2, {_spectral_lib.MAX_M}] = [{2 * ndim + 2}, {_spectral_lib.MAX_M}]")
    if not (float(tol) > 0 and np.isfinite(float(tol))):
        raise ValueError("tol must be positive and finite")
    if max_restarts < 0:
        raise ValueError("max_restarts must not be negative")
    if start is not None:
        start = np.ascontiguousarray(start, dtype=np.float64)
        if start.shape != (N, ndim):
            raise ValueError(f"start must be an N x ndim = {N} x {ndim} array")
        if not np.isfinite(start).all():
            raise ValueError("start must be finite")
    return ndim, m, max_restarts, start


def _spectral_solve(P, ndim=2, start=None, seed=18051982, tol=1e-4, m=32, max_restarts=200, device: int = 0) -> dict:
    """:func:`spectral_embedding` without its verdicts: a disconnected graph comes back with ``vectors`` None."""
    csr = _spectral_csr(P)
    N = csr[0]
    ndim, m, max_restarts, start = _spectral_args(N, ndim, m, tol, max_restarts, start)
    if start is None:
        start = np.random.default_rng(seed).standard_normal((N, ndim))
    ops = _umap_hip(device)
    tc, dev = ops.torch, f"cuda:{device}"
    _, cap, rowptr, col, val = _dev_csr(ops, csr, device)
    d_start = tc.from_numpy(start).to(dev)
    theta = tc.full((ndim,), float("nan"), dtype=tc.float64, device=dev)
    resid = tc.full((ndim,), float("nan"), dtype=tc.float64, device=dev)
    vectors = tc.empty((N, ndim), dtype=tc.float64, device=dev)
    info = tc.zeros(4, dtype=tc.int64, device=dev)
    ws = tc.empty(max(ops.spectral_workspace_bytes(N, cap, ndim, m), 1), dtype=tc.uint8, device=dev)
    ops.spectral(N, rowptr, col, val, cap, ndim, d_start, tol, m, max_restarts, ws, theta, resid, vectors, info)
    info = info.cpu().numpy()
    r = {"vectors": None, "values": None, "laplacian_values": None, "residuals": None, "n_components": int(info[0]),
         "restarts": int(info[1]), "multiplications": int(info[2]), "converged": bool(info[3])}
    if r["n_components"] == 1:
        th = theta.cpu().numpy()
        r.update(vectors=vectors.cpu().numpy(), values=th, laplacian_values=1.0 - th, residuals=resid.cpu().numpy())
    return r


def spectral_embedding(P, ndim: int = 2, start=None, seed: int = 18051982, tol: float = 1e-4, m: int = 32, max_restarts: int = 200,
                       device: int = 0) -> dict:
    """The ``ndim`` lowest non-trivial eigenvectors of the normalised Laplacian of the symmetric graph ``P`` (scipy sparse, as
    :func:`fuzzy_simplicial_set` returns it): ``gficf_spectral_device`` (include/gficf_spectral.h), a block Krylov subspace with
    thick restart in f64 on S = D^-1/2 P D^-1/2, in the complement of its trivial eigenvector.  ``start``: the N x ndim start block
    (default: standard normal from ``default_rng(seed)``); ``tol``: the bound on ``|S x - theta x| / |theta|`` (uwot's 1e-4); ``m``:
    the columns of the basis; ``max_restarts``.  Returns ``{"vectors": N x ndim float64 (unit columns, the largest-magnitude entry of
    each positive), "values": theta, "laplacian_values": 1 - theta, "residuals", "n_components", "restarts", "multiplications",
    "converged"}``.  Raises ``ValueError`` naming the number of components when the graph is disconnected; warns when the
    residuals do not meet ``tol`` after ``max_restarts`` restarts (what it has is returned)."""
    r = _spectral_solve(P, ndim, start, seed, tol, m, max_restarts, device)
    if r["n_components"] > 1:
        raise ValueError(f"the graph has {r['n_components']} connected components: its Laplacian eigenvectors are not an embedding "
                         "(see graph_components)")
    if not r["converged"]:
        warnings.warn(f"spectral_embedding: not converged after {r['restarts']} restarts (residuals {r['residuals']}, tol {tol})")
    return r


def _spectral_coordinates(vectors, rng, jitter: bool) -> np.ndarray:
    Y = np.array(vectors, dtype=np.float64)
    if jitter:
        top = np.abs(Y).max()
        if top > 0:
            Y *= 10.0 / top
        Y = Y + rng.normal(0.0, 1e-4, size=Y.shape)
    return Y


def spectral_init(P, seed: int = 18051982, jitter: bool = True, device: int = 0, **solver_kw) -> np.ndarray:
    """uwot's spectral start of the layout from the fuzzy graph ``P``, N x 2 float64: the two vectors of
    :func:`spectral_embedding`; with ``jitter`` (uwot's ``"spectral"``) scaled to a largest magnitude of 10 plus N(0, 1e-4) noise,
    the scaling of :func:`umap_init`'s ``"pca"``; without (uwot's ``"normlaplacian"``) the raw unit vectors.  One
    ``default_rng(seed)`` draws the start block first and the noise second.  ``solver_kw``: ``tol``, ``m``, ``max_restarts``."""
    N = _spectral_csr(P)[0]
    rng = np.random.default_rng(seed)
    if N <= 2:
        raise ValueError(f"N = {N} vertices for ndim = 2: N must exceed ndim")
    start = rng.standard_normal((N, 2))
    r = spectral_embedding(P, 2, start=start, device=device, **solver_kw)
    return _spectral_coordinates(r["vectors"], rng, jitter)


SPECTRAL_INITS = ("spectral", "normlaplacian")


def _umap_spectral(X, init, k, metric, n_epochs, learning_rate, a, b, negative_sample_rate, repulsion_strength, set_op_mix_ratio, local_connectivity,
                   seed, ret_graph, ret_nn, ctx) -> dict:
    """:func:`umap` from a spectral start: the stages one after the other (their bits are the chained call's)."""
    N = X.shape[0]
    nn = find_nn(X, k, True, metric, ctx=ctx)
    P = fuzzy_simplicial_set(nn["idx"], nn["dist"], set_op_mix_ratio, local_connectivity)[0]
    rng = np.random.default_rng(seed)
    r = _spectral_solve(P, 2, start=rng.standard_normal((N, 2)))
    if r["n_components"] > 1:
        warnings.warn(f"found more than one component ({r['n_components']}) in the graph: falling back to init='pca'")
        Y0 = umap_init("pca", X, N, seed)
    else:
        if not r["converged"]:
            warnings.warn(f"spectral initialisation not converged after {r['restarts']} restarts (residuals {r['residuals']})")
        Y0 = _spectral_coordinates(r["vectors"], rng, init == "spectral")
    Y = umap_layout(P, Y0, n_epochs, a, b, learning_rate, negative_sample_rate, repulsion_strength, seed=int(seed) & 0xFFFFFFFFFFFFFFFF)
    return {"embedding": Y.astype(np.float64), "graph": P if ret_graph else None,
            "nn": {"idx": nn["idx"], "dist": np.asarray(nn["dist"], dtype=np.float64)} if ret_nn else None, "a": float(a), "b": float(b),
            "n_neighbors": k, "metric": metric, "n_epochs": int(n_epochs), "seed": int(seed)}


def umap(X, init, n_neighbors: int = 15, metric: str = "euclidean", n_epochs: int | None = None, learning_rate: float = 1.0, a: float = 1.0,
         b: float = 1.0, negative_sample_rate: int = 5, repulsion_strength: float = 1.0, set_op_mix_ratio: float = 1.0,
         local_connectivity: float = 1.0, seed: int = 18051982, ret_graph: bool = True, ret_nn: bool = True, ctx: Context | None = None) -> dict:
    """The embedding of the rows of ``X`` (N x d, d <= 128) in one call of the C ABI (``gficf_umap_host``): exact neighbour
    search with distances, fuzzy graph, ``n_epochs`` layout sweeps from ``init`` (N x 2), all on the device.  ``n_neighbors``
    counts the point itself, as uwot's does.  Returns ``{"embedding": N x 2, "graph": scipy CSR, "nn": {"idx", "dist"}, "a",
    "b", "n_neighbors", "metric", "n_epochs", "seed"}`` (``graph`` / ``nn`` are None when not asked for).

    ``init`` may also be ``"spectral"`` (uwot's default: :func:`spectral_init` of the fuzzy graph) or ``"normlaplacian"`` (the same
    without scaling and noise).  The call then runs the stages one after the other, :func:`find_nn`, :func:`fuzzy_simplicial_set`,
    :func:`spectral_init`, :func:`umap_layout`, and returns the same dict.  A graph of more than one component warns, naming the
    count, and starts from ``umap_init("pca", X, N, seed)`` as uwot does: the result is that call's, bit for bit."""
    import scipy.sparse as sp

    from . import _umap_lib

    if metric not in _lib.KNN_METRICS:
        raise ValueError(f"metric must be one of {sorted(_lib.KNN_METRICS)}")
    X = np.asfortranarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("X must be a 2-d matrix")
    N, d = X.shape
    k = int(n_neighbors)
    if n_epochs is None:
        n_epochs = 500 if N <= 10000 else 200
    if isinstance(init, str):
        if init not in SPECTRAL_INITS:
            raise ValueError(f"init must be an N x 2 array or one of {SPECTRAL_INITS}")
        return _umap_spectral(X, init, k, metric, n_epochs, learning_rate, a, b, negative_sample_rate, repulsion_strength, set_op_mix_ratio,
                              local_connectivity, seed, ret_graph, ret_nn, ctx)
    Y0 = np.asfortranarray(init, dtype=np.float64)
    if Y0.shape != (N, 2):
        raise ValueError(f"init must be an N x 2 = {N} x 2 array")
    emb = np.zeros((2, N), dtype=np.float64)                  # C-order (2, N) == column-major N x 2
    cap = max(2 * N * max(k, 0), 1)
    rowptr = col = val = nnz = idx = dist = None
    if ret_graph:
        rowptr, col, val, nnz = np.zeros(N + 1, np.int64), np.zeros(cap, np.int32), np.zeros(cap, np.float32), np.zeros(1, np.int64)
    if ret_nn:
        idx, dist = np.zeros((max(k, 1), N), np.int32), np.zeros((max(k, 1), N), np.float32)
    ctx = ctx or default_context()
    check(_umap_lib.load().gficf_umap_host(ctx.handle, _np_ptr(X), N, d, max(N, 1), _lib.KNN_METRICS[metric], k, float(local_connectivity),
                                           float(set_op_mix_ratio), float(a), float(b), float(repulsion_strength), float(learning_rate),
                                           int(negative_sample_rate), int(n_epochs), _np_ptr(Y0), int(seed) & 0xFFFFFFFFFFFFFFFF, _np_ptr(emb),
                                           _np_ptr(rowptr), _np_ptr(col), _np_ptr(val), _np_ptr(nnz), _np_ptr(idx), _np_ptr(dist)))
    graph = nn = None
    if ret_graph:
        n = int(nnz[0])
        graph = sp.csr_matrix((val[:n].copy(), col[:n].copy(), rowptr), shape=(N, N))
    if ret_nn:
        nn = {"idx": np.ascontiguousarray(idx.T), "dist": np.ascontiguousarray(dist.T, dtype=np.float64)}
    return {"embedding": np.ascontiguousarray(emb.T), "graph": graph, "nn": nn, "a": float(a), "b": float(b), "n_neighbors": k,
            "metric": metric, "n_epochs": int(n_epochs), "seed": int(seed)}


def runReduction(data: dict, reduction: str = "tumap", nt: int = 2, seed: int = 18051982, ret_model_pred: bool = True, verbose: bool = True,
                 ctx: Context | None = None, **kw) -> dict:
    """``runReduction(data, reduction, nt, seed, ret_model_pred, verbose, ...)`` of the reference
    (R/dimensinalityReduction.R:157-192, whose default is ``uwot::tumap(data$pca$cells)``) on the device (:func:`umap`).  RELAXED
    CONTRACT (include/gficf_umap.h): the algorithm and its objective are UMAP's, the random bits and the update order are not
    uwot's.  Further arguments, with uwot's meaning: ``n_neighbors=15, metric="euclidean", n_epochs=None`` (500 for N <= 10 000,
    else 200), ``learning_rate=1, min_dist=0.01, spread=1, a=None, b=None, negative_sample_rate=5, repulsion_strength=1,
    set_op_mix_ratio=1, local_connectivity=1, init="pca"`` (:func:`umap_init`, or ``"normlaplacian"``: the Laplacian eigenvectors
    of the graph through :func:`umap`; uwot's default ``"spectral"`` is provided by ``gficf_amd.umap(..., init="spectral")`` and
    :func:`spectral_init`, and still raises here: the default stays ``"pca"``, the one divergence in defaults).  ``"tumap"`` is a = b = 1; ``"umap"`` fits them (:func:`find_ab_params`) unless both are given.

    ``data["embedded"]`` becomes a pandas DataFrame with the columns ``X`` and ``Y`` (what ``clustcells(from_embedded=True)``
    searches), ``data["reduction"]`` the name, and with ``ret_model_pred`` ``data["uwot"]`` the dict of :func:`umap`.  Not provided,
    each raising ``NotImplementedError``: ``reduction="tsne"``, ``init="spectral"``, and a ``data`` without ``data["pca"]`` (the
    reference then embeds ``t(gficf)`` itself: :func:`runReductionSparse` does, and the message names it).  ``nt`` is accepted for
    signature compatibility (no CPU threads)."""
    import pandas as pd

    if reduction == "tsne":
        raise NotImplementedError("reduction='tsne' (Rtsne) is not provided by runReduction: use 'tumap' or 'umap', or call runTsne")
    if reduction not in REDUCTIONS:
        raise ValueError(f"reduction must be one of {REDUCTIONS} ('tsne' is not provided)")
    unknown = sorted(set(kw) - set(_REDUCTION_KW))
    if unknown:
        raise TypeError(f"runReduction: unknown argument(s) {unknown}")
    o = dict(_REDUCTION_KW, **kw)
    if data.get("pca") is None:
        raise NotImplementedError("runReduction without data['pca'] (the reference embeds the densified t(gficf)) is not provided: "
                                  "run runPCA or runLSA first, or call runReductionSparse, which searches the sparse cells")
    if o["metric"] not in _lib.KNN_METRICS:
        raise ValueError(f"metric must be one of {sorted(_lib.KNN_METRICS)}")
    cells = np.asarray(data["pca"]["cells"], dtype=np.float64)
    N = cells.shape[0]
    Y0 = "normlaplacian" if isinstance(o["init"], str) and o["init"] == "normlaplacian" else umap_init(o["init"], cells, N, seed)
    if reduction == "tumap":
        a = b = 1.0
    elif o["a"] is not None and o["b"] is not None:
        a, b = float(o["a"]), float(o["b"])
    else:
        a, b = find_ab_params(o["spread"], o["min_dist"])
    tsmessage(f"Running {reduction} on {N} cells, {cells.shape[1]} components", verbose=verbose)
    r = umap(cells, Y0, n_neighbors=o["n_neighbors"], metric=o["metric"], n_epochs=o["n_epochs"], learning_rate=o["learning_rate"], a=a, b=b,
             negative_sample_rate=o["negative_sample_rate"], repulsion_strength=o["repulsion_strength"], set_op_mix_ratio=o["set_op_mix_ratio"],
             local_connectivity=o["local_connectivity"], seed=seed, ret_graph=bool(ret_model_pred), ret_nn=bool(ret_model_pred), ctx=ctx)
    data["embedded"] = pd.DataFrame(r["embedding"], columns=["X", "Y"])
    data["reduction"] = reduction
    if ret_model_pred:
        data["uwot"] = r
    return data


# ------------------------------------------------------------------ t-SNE (libgficf_tsne.so)
_TSNE_KW = {"perplexity": 30, "theta": 0.5, "max_iter": 1000, "Y_init": None, "normalize": True, "stop_lying_iter": None,
            "mom_switch_iter": None, "momentum": 0.5, "final_momentum": 0.8, "eta": 200, "exaggeration_factor": 12, "ret_P": False,
            "ret_nn": False}


def _tsne_k(perplexity, N: int) -> int:
    """The columns of the neighbour table for ``perplexity`` (floor(3 perplexity) + 1), after the checks of include/gficf_tsne.h
    that need no device: the library would say the same."""
    perplexity = float(perplexity)
    if not perplexity > 0 or not np.isfinite(perplexity):
        raise ValueError("perplexity must be positive")
    if N - 1 < 3 * perplexity:
        raise ValueError(f"perplexity = {perplexity:g} is too large for the number of samples ({N}): N - 1 >= 3 perplexity")
    K = int(np.floor(3 * perplexity))
    if K + 1 > _lib.KNN_MAX_K:
        raise GficfError(6, f"perplexity = {perplexity:g} needs {K + 1} neighbours, beyond {_lib.KNN_MAX_K} (perplexity < 42.34)")
    if K < 1:
        raise ValueError(f"perplexity = {perplexity:g} names no neighbour (floor(3 perplexity) = 0)")
    return K + 1


def _tsne_dev_csr(ops, P):
    csr = _square_csr(P, allow_arrays=True)
    if csr[0] < 1 or len(csr[3]) != len(csr[2]):
        raise ValueError("P needs at least one row, and as many values as columns")
    return _dev_csr(ops, csr, ops.device)


def _tsne_state(a, N: int, name: str, fill: float) -> np.ndarray:
    if a is None:
        return np.full((N, 2), fill, dtype=np.float32)
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.shape != (N, 2):
        raise ValueError(f"{name} must be an N x 2 = {N} x 2 array")
    return a


def tsne_shape(N: int) -> dict:
    """The decomposition of the repulsion kernel for ``N`` points (``gficf_tsne_shape``, a host query that depends on N only):
    ``{"rows_per_block", "tile", "slices"}``.  ``tile`` is also T, the longest f32 accumulation chain (include/gficf_tsne.h)."""
    from . import _tsne_lib

    r, t, s = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    check(_tsne_lib.load().gficf_tsne_shape(int(N), ctypes.byref(r), ctypes.byref(t), ctypes.byref(s)))
    return {"rows_per_block": r.value, "tile": t.value, "slices": s.value}


def tsne_affinities(idx, dist, perplexity: float = 30, ret_cond: bool = False, device: int = 0):
    """t-SNE's input similarities from a euclidean neighbour table as :func:`find_nn` returns it (``idx`` N x k, 1-based, column 0
    the point itself; ``dist`` alike; the first ``floor(3 perplexity) + 1`` columns are used): the bisection for every row's
    ``beta`` and the symmetrisation ``(Pc + Pc') / (2 N)`` (``gficf_tsne_affinities_device``, include/gficf_tsne.h).  Returns
    ``(P, beta)``: the N x N scipy CSR matrix (float32, columns ascending, ``P == P.T`` bit for bit) and the float64 vector; with
    ``ret_cond`` also ``Pc``, the N x floor(3 perplexity) float32 conditionals before the symmetrisation."""
    import scipy.sparse as sp

    idx, dist = np.asarray(idx), np.asarray(dist)
    if idx.ndim != 2 or idx.shape != dist.shape:
        raise ValueError("idx and dist must be N x k matrices of the same shape")
    N = idx.shape[0]
    k = _tsne_k(perplexity, N)
    if idx.shape[1] < k:
        raise ValueError(f"perplexity = {float(perplexity):g} needs a table of floor(3 perplexity) + 1 = {k} columns, got {idx.shape[1]}")
    K = k - 1
    ops = _umap_hip(device)
    tc, dev = ops.torch, f"cuda:{device}"
    d_idx = tc.from_numpy(np.ascontiguousarray(idx[:, :k].T, dtype=np.int32)).to(dev)    # (k, N) C-order == column-major N x k
    d_dist = tc.from_numpy(np.ascontiguousarray(dist[:, :k].T, dtype=np.float32)).to(dev)
    cap = 2 * N * K
    ws = tc.empty(max(ops.tsne_affinities_workspace_bytes(N, k), 1), dtype=tc.uint8, device=dev)
    rowptr = tc.empty(N + 1, dtype=tc.int64, device=dev)
    col = tc.empty(cap, dtype=tc.int32, device=dev)
    val = tc.empty(cap, dtype=tc.float32, device=dev)
    nnz = tc.zeros(1, dtype=tc.int64, device=dev)
    beta = tc.empty(N, dtype=tc.float64, device=dev)
    pc = tc.empty((K, N), dtype=tc.float32, device=dev) if ret_cond else None
    ops.tsne_affinities(d_idx, d_dist, N, k, perplexity, ws, rowptr, col, val, nnz, beta, pc)
    ops.tsne_sync(ws)
    n = int(nnz.item())
    P = sp.csr_matrix((val[:n].cpu().numpy(), col[:n].cpu().numpy(), rowptr.cpu().numpy()), shape=(N, N))
    if ret_cond:
        return P, beta.cpu().numpy(), np.ascontiguousarray(pc.cpu().numpy().T)
    return P, beta.cpu().numpy()


def tsne_gradient(P, Y, exaggeration: float = 1.0, device: int = 0) -> dict:
    """One evaluation of t-SNE's gradient at the coordinates ``Y`` (N x 2) over ``P`` (scipy sparse, or ``(indptr, indices,
    data)``): ``gficf_tsne_gradient_device``, the exact repulsive field of all N^2 pairs.  Returns ``{"grad": N x 2 float32 (x
    attr - rep / Z: Rtsne's form, without the factor 4), "rep": N x 2 float32 (un-normalised), "Z": float, "kl": float}``."""
    ops = _umap_hip(device)
    tc, dev = ops.torch, f"cuda:{device}"
    N, cap, rowptr, col, val = _tsne_dev_csr(ops, P)
    d_Y = tc.from_numpy(_tsne_state(Y, N, "Y", 0.0)).to(dev)
    ws = tc.empty(max(ops.tsne_layout_workspace_bytes(N, cap), 1), dtype=tc.uint8, device=dev)
    dC = tc.empty((N, 2), dtype=tc.float32, device=dev)
    rep = tc.empty((N, 2), dtype=tc.float32, device=dev)
    zk = tc.zeros(2, dtype=tc.float64, device=dev)
    ops.tsne_gradient(N, rowptr, col, val, cap, d_Y, exaggeration, ws, dC, rep, zk[0:1], zk[1:2])
    ops.tsne_sync(ws)
    zk = zk.cpu().numpy()
    return {"grad": dC.cpu().numpy(), "rep": rep.cpu().numpy(), "Z": float(zk[0]), "kl": float(zk[1])}


def tsne_layout(P, Y, max_iter: int = 1000, iter_begin: int = 0, iter_end=None, uY=None, gains=None, stop_lying_iter: int = 250,
                mom_switch_iter: int = 250, momentum: float = 0.5, final_momentum: float = 0.8, eta: float = 200,
                exaggeration_factor: float = 12, ret_state: bool = False, ret_kl: bool = False, device: int = 0):
    """Iterations ``[iter_begin, iter_end)`` of ``max_iter`` of the t-SNE layout over ``P`` from the coordinates ``Y`` (N x 2):
    ``gficf_tsne_layout_device``, the update rule of include/gficf_tsne.h.  ``uY`` (the velocity, default 0) and ``gains`` (default
    1) are the rest of the state.  Returns the N x 2 float32 coordinates, or with ``ret_state`` the tuple ``(Y, uY, gains)``;
    handing the three back and running ``[a, n)`` after ``[0, a)`` gives the bits of ``[0, n)``.  ``ret_kl`` appends the KL
    divergence of the coordinates returned."""
    ops = _umap_hip(device)
    tc, dev = ops.torch, f"cuda:{device}"
    N, cap, rowptr, col, val = _tsne_dev_csr(ops, P)
    iter_end = int(max_iter) if iter_end is None else int(iter_end)
    d_Y = tc.from_numpy(_tsne_state(Y, N, "Y", 0.0)).to(dev)
    d_u = tc.from_numpy(_tsne_state(uY, N, "uY", 0.0)).to(dev)
    d_g = tc.from_numpy(_tsne_state(gains, N, "gains", 1.0)).to(dev)
    ws = tc.empty(max(ops.tsne_layout_workspace_bytes(N, cap), 1), dtype=tc.uint8, device=dev)
    kl = tc.zeros(1, dtype=tc.float64, device=dev) if ret_kl else None
    ops.tsne_layout(N, rowptr, col, val, cap, max_iter, iter_begin, iter_end, stop_lying_iter, mom_switch_iter, momentum, final_momentum, eta,
                    exaggeration_factor, d_Y, d_u, d_g, ws, kl)
    ops.tsne_sync(ws)
    out = (d_Y.cpu().numpy(), d_u.cpu().numpy(), d_g.cpu().numpy()) if ret_state else d_Y.cpu().numpy()
    if ret_kl:
        return (*out, float(kl.item())) if ret_state else (out, float(kl.item()))
    return out


def Rtsne(X, dims: int = 2, perplexity: float = 30, theta: float = 0.5, max_iter: int = 1000, Y_init=None, normalize: bool = True,
          stop_lying_iter=None, mom_switch_iter=None, momentum: float = 0.5, final_momentum: float = 0.8, eta: float = 200,
          exaggeration_factor: float = 12, pca: bool = False, seed: int = 18051982, ret_P: bool = False, ret_nn: bool = False,
          ctx: Context | None = None) -> dict:
    """``Rtsne::Rtsne(X, dims = 2, pca = F, ...)`` on the device in one call of the C ABI (``gficf_tsne_host``): exact euclidean
    neighbour search (``floor(3 perplexity)`` neighbours), the perplexity graph, ``max_iter`` iterations of the layout with the
    EXACT repulsion of all N^2 pairs.  RELAXED CONTRACT (include/gficf_tsne.h): the algorithm and its objective are Rtsne's, the
    random bits are not: without ``Y_init`` the start is ``default_rng(seed).standard_normal((N, 2)) * 1e-4``.

    ``normalize`` is Rtsne's ``normalize_input`` (the columns centred, then everything divided by the largest magnitude), done
    on the host.  ``theta`` is accepted and recorded: the repulsion is exact whatever its value.  ``stop_lying_iter`` and
    ``mom_switch_iter`` default to 250, or to 0 when ``Y_init`` is given, as in Rtsne.  ``dims != 2`` and ``pca=True`` (Rtsne's
    own PCA step; the reference passes ``pca = F``) raise ``ValueError``.  Duplicate rows are not checked for (Rtsne refuses
    them): they are harmless here.  Returns ``{"Y": N x 2, "N", "perplexity", "costs": the final KL divergence, "theta",
    "max_iter", "eta", "stop_lying_iter", "mom_switch_iter", "momentum", "final_momentum", "exaggeration_factor", "P": scipy CSR
    or None, "nn": {"idx", "dist"} or None}``."""
    import scipy.sparse as sp

    from . import _tsne_lib

    if int(dims) != 2:
        raise ValueError("dims must be 2: the layout is two-dimensional")
    if pca:
        raise ValueError("pca=True (Rtsne's own PCA step) is not provided: pass the components (the reference calls Rtsne with pca = F)")
    X = np.array(X, dtype=np.float64, order="F")
    if X.ndim != 2:
        raise ValueError("X must be a 2-d matrix")
    N, d = X.shape
    k = _tsne_k(perplexity, N)
    given = Y_init is not None
    if given:
        Y0 = np.asfortranarray(Y_init, dtype=np.float64)
        if Y0.shape != (N, 2):
            raise ValueError(f"Y_init must be an N x 2 = {N} x 2 array")
    else:
        Y0 = np.asfortranarray(np.random.default_rng(seed).standard_normal((N, 2)) * 1e-4)
    stop_lying_iter = (0 if given else 250) if stop_lying_iter is None else int(stop_lying_iter)
    mom_switch_iter = (0 if given else 250) if mom_switch_iter is None else int(mom_switch_iter)
    if normalize:
        X -= X.mean(axis=0)
        top = np.abs(X).max()
        if top > 0:
            X /= top
    emb = np.zeros((2, N), dtype=np.float64)                  # C-order (2, N) == column-major N x 2
    kl = np.zeros(1, dtype=np.float64)
    cap = 2 * N * (k - 1)
    rowptr = col = val = nnz = idx = dist = None
    if ret_P:
        rowptr, col, val, nnz = np.zeros(N + 1, np.int64), np.zeros(cap, np.int32), np.zeros(cap, np.float32), np.zeros(1, np.int64)
    if ret_nn:
        idx, dist = np.zeros((k, N), np.int32), np.zeros((k, N), np.float32)
    ctx = ctx or default_context()
    check(_tsne_lib.load().gficf_tsne_host(ctx.handle, _np_ptr(X), N, d, max(N, 1), float(perplexity), int(max_iter), stop_lying_iter,
                                           mom_switch_iter, float(momentum), float(final_momentum), float(eta), float(exaggeration_factor),
                                           _np_ptr(Y0), _np_ptr(emb), _np_ptr(kl), _np_ptr(rowptr), _np_ptr(col), _np_ptr(val), _np_ptr(nnz),
                                           _np_ptr(idx), _np_ptr(dist)))
    P = nn = None
    if ret_P:
        n = int(nnz[0])
        P = sp.csr_matrix((val[:n].copy(), col[:n].copy(), rowptr), shape=(N, N))
    if ret_nn:
        nn = {"idx": np.ascontiguousarray(idx.T), "dist": np.ascontiguousarray(dist.T, dtype=np.float64)}
    return {"Y": np.ascontiguousarray(emb.T), "N": N, "perplexity": float(perplexity), "costs": float(kl[0]), "theta": float(theta),
            "max_iter": int(max_iter), "eta": float(eta), "stop_lying_iter": stop_lying_iter, "mom_switch_iter": mom_switch_iter,
            "momentum": float(momentum), "final_momentum": float(final_momentum), "exaggeration_factor": float(exaggeration_factor), "P": P,
            "nn": nn}


def runTsne(data: dict, seed: int = 18051982, verbose: bool = True, ctx: Context | None = None, **kw) -> dict:
    """The ``reduction = "tsne"`` branch of the reference's ``runReduction`` (R/dimensinalityReduction.R:175-177:
    ``Rtsne::Rtsne(X = data$pca$cells, dims = 2, pca = F, max_iter = 1000)``) on the device (:func:`Rtsne`, whose further
    arguments are accepted here with Rtsne's defaults: ``perplexity=30, theta=0.5, max_iter=1000, Y_init=None, normalize=True,
    stop_lying_iter=None, mom_switch_iter=None, momentum=0.5, final_momentum=0.8, eta=200, exaggeration_factor=12, ret_P=False,
    ret_nn=False``).  ``data["embedded"]`` becomes a pandas DataFrame with the columns ``X`` and ``Y``, ``data["reduction"]``
    ``"tsne"`` and ``data["uwot"]`` None, as the reference leaves them; ``data["tsne"]`` keeps the rest of what :func:`Rtsne`
    returned.  A ``data`` without ``data["pca"]`` raises ``NotImplementedError`` (the reference then embeds ``t(gficf)`` itself:
    ``runReductionSparse(reduction="tsne")`` does, and the message names it)."""
    import pandas as pd

    unknown = sorted(set(kw) - set(_TSNE_KW))
    if unknown:
        raise TypeError(f"runTsne: unknown argument(s) {unknown}")
    if data.get("pca") is None:
        raise NotImplementedError("runTsne without data['pca'] (the reference embeds the densified t(gficf)) is not provided: "
                                  "run runPCA or runLSA first, or call runReductionSparse(reduction='tsne'), which searches the sparse cells")
    cells = np.asarray(data["pca"]["cells"], dtype=np.float64)
    tsmessage(f"Running tsne on {cells.shape[0]} cells, {cells.shape[1]} components", verbose=verbose)
    r = Rtsne(cells, dims=2, pca=False, seed=seed, ctx=ctx, **dict(_TSNE_KW, **kw))
    data["embedded"] = pd.DataFrame(r.pop("Y"), columns=["X", "Y"])
    data["reduction"] = "tsne"
    data["uwot"] = None
    data["tsne"] = r
    return data


# ------------------------------------------------------------------ embedding without PCA (libgficf_sparse_knn.so)
SPARSE_REDUCTIONS = ("tumap", "umap", "tsne")


def _sparse_centred_top(M) -> float:
    """The largest magnitude of ``t(M)`` after its columns (the genes) are centred, without densifying it: Rtsne's
    ``normalize_input`` divides by it, and centring itself moves no euclidean distance."""
    import scipy.sparse as sp

    M = sp.csc_matrix(M)
    G, N = M.shape
    mean = np.asarray(M.sum(axis=1)).ravel() / N
    top = float(np.abs(M.data - mean[M.indices]).max()) if M.nnz else 0.0
    absent = np.bincount(M.indices, minlength=G) < N               # genes some cell does not store: that cell holds -mean
    return max(top, float(np.abs(mean[absent]).max()) if absent.any() else 0.0)


def _reduction_sparse_umap(M, reduction, o, seed, ret_model_pred, ctx) -> dict:
    N = M.shape[1]
    k = int(o["n_neighbors"])
    n_epochs = (500 if N <= 10000 else 200) if o["n_epochs"] is None else int(o["n_epochs"])
    if reduction == "tumap":
        a = b = 1.0
    elif o["a"] is not None and o["b"] is not None:
        a, b = float(o["a"]), float(o["b"])
    else:
        a, b = find_ab_params(o["spread"], o["min_dist"])
    init = o["init"]
    if isinstance(init, str) and init not in SPECTRAL_INITS + ("pca", "random"):
        raise ValueError(f"init must be an N x 2 array or one of {SPECTRAL_INITS + ('pca', 'random')}")
    nn = find_nn_sparse(M, k, True, o["metric"], ctx=ctx)
    P = fuzzy_simplicial_set(nn["idx"], nn["dist"], o["set_op_mix_ratio"], o["local_connectivity"])[0]

    def pca_start():
        return umap_init("pca", rsvd(M, k=2, centre=True, ctx=ctx)["cells"], N, seed)

    if isinstance(init, str) and init in SPECTRAL_INITS:
        rng = np.random.default_rng(seed)
        r = _spectral_solve(P, 2, start=rng.standard_normal((N, 2)))
        if r["n_components"] > 1:
            warnings.warn(f"found more than one component ({r['n_components']}) in the graph: falling back to init='pca'")
            Y0 = pca_start()
        else:
            if not r["converged"]:
                warnings.warn(f"spectral initialisation not converged after {r['restarts']} restarts (residuals {r['residuals']})")
            Y0 = _spectral_coordinates(r["vectors"], rng, init == "spectral")
    elif isinstance(init, str) and init == "pca":
        Y0 = pca_start()
    else:
        Y0 = umap_init(init, None, N, seed)
    Y = umap_layout(P, Y0, n_epochs, a, b, o["learning_rate"], o["negative_sample_rate"], o["repulsion_strength"],
                    seed=int(seed) & 0xFFFFFFFFFFFFFFFF)
    return {"embedding": Y.astype(np.float64), "graph": P if ret_model_pred else None, "nn": nn if ret_model_pred else None, "a": float(a),
            "b": float(b), "n_neighbors": k, "metric": o["metric"], "n_epochs": n_epochs, "seed": int(seed), "space": "gficf"}


def _reduction_sparse_tsne(M, o, seed, ctx) -> dict:
    N = M.shape[1]
    k = _tsne_k(o["perplexity"], N)
    given = o["Y_init"] is not None
    Y0 = _tsne_state(o["Y_init"], N, "Y_init", 0.0) if given else np.random.default_rng(seed).standard_normal((N, 2)) * 1e-4
    stop_lying_iter = (0 if given else 250) if o["stop_lying_iter"] is None else int(o["stop_lying_iter"])
    mom_switch_iter = (0 if given else 250) if o["mom_switch_iter"] is None else int(o["mom_switch_iter"])
    nn = find_nn_sparse(M, k, True, "euclidean", ctx=ctx)
    if o["normalize"]:
        top = _sparse_centred_top(M)
        if top > 0:
            nn["dist"] = nn["dist"] / top
    P = tsne_affinities(nn["idx"], nn["dist"], o["perplexity"])[0]
    Y, kl = tsne_layout(P, Y0, int(o["max_iter"]), stop_lying_iter=stop_lying_iter, mom_switch_iter=mom_switch_iter, momentum=o["momentum"],
                        final_momentum=o["final_momentum"], eta=o["eta"], exaggeration_factor=o["exaggeration_factor"], ret_kl=True)
    return {"Y": Y.astype(np.float64), "N": N, "perplexity": float(o["perplexity"]), "costs": kl, "theta": float(o["theta"]),
            "max_iter": int(o["max_iter"]), "eta": float(o["eta"]), "stop_lying_iter": stop_lying_iter, "mom_switch_iter": mom_switch_iter,
            "momentum": float(o["momentum"]), "final_momentum": float(o["final_momentum"]), "exaggeration_factor": float(o["exaggeration_factor"]),
            "P": P if o["ret_P"] else None, "nn": nn if o["ret_nn"] else None, "space": "gficf"}


def runReductionSparse(data: dict, reduction: str = "tumap", seed: int = 18051982, ret_model_pred: bool = True, verbose: bool = True,
                       ctx: Context | None = None, **kw) -> dict:
    """The ``data$pca``-less branch of the reference's ``runReduction`` (R/dimensinalityReduction.R:179-187: ``tumap``, ``umap``
    or ``Rtsne`` of ``t(data$gficf)``) on the device, composed from the stages the package has; the cells are never densified:
    the neighbour search is :func:`find_nn_sparse` over the columns of ``data["gficf"]``.

    ``"tumap"`` / ``"umap"``: :func:`find_nn_sparse` -> :func:`fuzzy_simplicial_set` -> start -> :func:`umap_layout`, with
    :func:`runReduction`'s keywords.  ``init`` is ``"spectral"`` (the default HERE, as uwot's: :func:`spectral_init`'s solve of the
    graph; a graph of more than one component warns, naming the count, and starts from ``"pca"``), ``"normlaplacian"``,
    ``"pca"`` (``rsvd(data["gficf"], k=2, centre=True)["cells"]`` through :func:`umap_init`'s scaling), ``"random"`` or an N x 2
    array.  ``"tsne"``: ``find_nn_sparse(euclidean, floor(3 perplexity) + 1)`` -> :func:`tsne_affinities` ->
    :func:`tsne_layout`, with :func:`runTsne`'s keywords and start; ``normalize`` divides the distances by the largest magnitude
    of the gene-centred matrix, which is what Rtsne's ``normalize_input`` does to them.

    ``data["embedded"]``, ``data["reduction"]`` and ``data["uwot"]`` (``data["tsne"]`` for t-SNE) are set as :func:`runReduction`
    and :func:`runTsne` set them; the model carries ``"space": "gficf"`` and its ``nn`` table.  :func:`embedNewCells` refuses such
    a model (the reference's needs ``data$pca`` too): :func:`embedNewCellsSparse` takes it."""
    import pandas as pd

    if reduction not in SPARSE_REDUCTIONS:
        raise ValueError(f"reduction must be one of {SPARSE_REDUCTIONS}")
    defaults = _TSNE_KW if reduction == "tsne" else dict(_REDUCTION_KW, init="spectral")
    unknown = sorted(set(kw) - set(defaults))
    if unknown:
        raise TypeError(f"runReductionSparse: unknown argument(s) {unknown}")
    o = dict(defaults, **kw)
    if data.get("gficf") is None:
        raise ValueError("runReductionSparse needs data['gficf']: run gficf first")
    if reduction != "tsne" and o["metric"] not in _lib.KNN_METRICS:
        raise ValueError(f"metric must be one of {sorted(_lib.KNN_METRICS)}")
    M = data["gficf"]
    tsmessage(f"Running {reduction} on {M.shape[1]} cells, {M.shape[0]} genes (sparse)", verbose=verbose)
    if reduction == "tsne":
        r = _reduction_sparse_tsne(M, o, seed, ctx)
        data["embedded"] = pd.DataFrame(r.pop("Y"), columns=["X", "Y"])
        data["uwot"] = None
        data["tsne"] = r
    else:
        r = _reduction_sparse_umap(M, reduction, o, seed, ret_model_pred, ctx)
        data["embedded"] = pd.DataFrame(r["embedding"], columns=["X", "Y"])
        if ret_model_pred:
            data["uwot"] = r
    data["reduction"] = reduction
    return data


# ------------------------------------------------------------------ new cells (libgficf_transform.so)
def _query_pair(X_train, Q):
    X = np.asfortranarray(X_train, dtype=np.float64)
    Qm = np.asfortranarray(Q, dtype=np.float64)
    if X.ndim != 2 or Qm.ndim != 2:
        raise ValueError("X_train and Q must be 2-d matrices")
    if X.shape[1] != Qm.shape[1]:
        raise ValueError(f"Q has {Qm.shape[1]} columns, X_train has {X.shape[1]}")
    return X, Qm


def find_nn_query(X_train, Q, k: int, metric: str = "euclidean", ctx: Context | None = None) -> dict:
    """The ``k`` nearest rows of ``X_train`` (N x d) for every row of ``Q`` (M x d): exact, f32, the arithmetic and the tie rule
    of :func:`find_nn` (``gficf_transform_search_host``, include/gficf_transform.h), so ``find_nn_query(X, X, k)`` is
    ``find_nn(X, k, True)`` bit for bit.  Returns ``{"idx": M x k int32, 1-based ids of training rows, "dist": M x k float64}``."""
    from . import _transform_lib

    if metric not in _lib.KNN_METRICS:
        raise ValueError(f"metric must be one of {sorted(_lib.KNN_METRICS)}")
    X, Qm = _query_pair(X_train, Q)
    (N, d), M, k = X.shape, Qm.shape[0], int(k)
    idx = np.zeros((max(k, 1), M), dtype=np.int32)            # C-order (k, M) == column-major M x k
    dist = np.zeros((max(k, 1), M), dtype=np.float64)
    ctx = ctx or default_context()
    check(_transform_lib.load().gficf_transform_search_host(ctx.handle, _np_ptr(X), N, max(N, 1), _np_ptr(Qm), M, max(M, 1), d, k,
                                                            _lib.KNN_METRICS[metric], _np_ptr(idx), _np_ptr(dist)))
    return {"idx": np.ascontiguousarray(idx.T), "dist": np.ascontiguousarray(dist.T)}


def umap_transform(Q, model: dict, X_train, n_epochs: int | None = None, learning_rate: float | None = None, negative_sample_rate: int = 5,
                   repulsion_strength: float = 1.0, local_connectivity: float = 1.0, seed: int | None = None, init="weighted",
                   query_offset: int = 0, epoch_begin: int = 0, epoch_end: int | None = None, ret_extra: bool = False,
                   ctx: Context | None = None):
    """``uwot::umap_transform`` for the rows of ``Q`` (M x d): their place in the plane of ``model``, the dict of :func:`umap`
    as :func:`runReduction` stores it in ``data["uwot"]``, trained on ``X_train`` (N x d) — one call of the C ABI
    (``gficf_transform_host``): search against the training rows, memberships, weighted initial positions, layout sweeps in
    which only the new cells move.  RELAXED CONTRACT (include/gficf_transform.h).

    From the model: ``embedding``, ``a``, ``b``, ``n_neighbors``, ``metric``, ``n_epochs``, ``seed``.  ``n_epochs=None`` means
    ``max(1, round(model["n_epochs"] / 3))``; ``learning_rate=None`` means 0.25, a quarter of the training default, as
    umap-learn's transform takes it; ``seed=None`` the model's.  The model does not record ``learning_rate``,
    ``negative_sample_rate``, ``repulsion_strength`` or ``local_connectivity``: a caller who trained with other values passes
    them again.  ``init``: ``"weighted"`` or an M x 2 array.  The result for row i depends on that row, the model and
    ``query_offset + i`` only: a batch may be cut into pieces.  Returns M x 2 float64; with ``ret_extra`` a dict with
    ``embedding``, ``idx``, ``dist``, ``w``, ``sigma``, ``rho`` and ``init`` (the positions the sweeps started from)."""
    from . import _transform_lib

    X, Qm = _query_pair(X_train, Q)
    (N, d), M = X.shape, Qm.shape[0]
    Yt = np.asfortranarray(model["embedding"], dtype=np.float64)
    if Yt.shape != (N, 2):
        raise ValueError(f"model['embedding'] must be N x 2 = {N} x 2: X_train is not what the model was trained on")
    metric, k = model["metric"], int(model["n_neighbors"])
    if metric not in _lib.KNN_METRICS:
        raise ValueError(f"metric must be one of {sorted(_lib.KNN_METRICS)}")
    if n_epochs is None:
        n_epochs = max(1, int(round(model["n_epochs"] / 3)))
    epoch_end = int(n_epochs) if epoch_end is None else int(epoch_end)
    learning_rate = 0.25 if learning_rate is None else float(learning_rate)
    seed = int(model["seed"]) if seed is None else int(seed)
    Y0 = None
    if not (isinstance(init, str) and init == "weighted"):
        if isinstance(init, str):
            raise ValueError("init must be 'weighted' or an M x 2 array")
        Y0 = np.asfortranarray(init, dtype=np.float64)
        if Y0.shape != (M, 2):
            raise ValueError(f"init must be 'weighted' or an M x 2 = {M} x 2 array")
    emb = np.zeros((2, M), dtype=np.float64)                  # C-order (2, M) == column-major M x 2
    idx = dist = w = sigma = rho = y0 = None
    if ret_extra:
        idx, dist, w = (np.zeros((max(k, 1), M), t) for t in (np.int32, np.float32, np.float32))
        sigma, rho, y0 = np.zeros(M, np.float32), np.zeros(M, np.float32), np.zeros((2, M), np.float64)
    ctx = ctx or default_context()
    check(_transform_lib.load().gficf_transform_host(
        ctx.handle, _np_ptr(X), N, max(N, 1), _np_ptr(Yt), _np_ptr(Qm), M, max(M, 1), d, _lib.KNN_METRICS[metric], k, float(local_connectivity),
        float(model["a"]), float(model["b"]), float(repulsion_strength), learning_rate, int(negative_sample_rate), int(n_epochs),
        int(epoch_begin), epoch_end, _np_ptr(Y0), seed & 0xFFFFFFFFFFFFFFFF, int(query_offset), _np_ptr(emb), _np_ptr(idx), _np_ptr(dist),
        _np_ptr(w), _np_ptr(sigma), _np_ptr(rho), _np_ptr(y0)))
    emb = np.ascontiguousarray(emb.T)
    if not ret_extra:
        return emb
    return {"embedding": emb, "idx": np.ascontiguousarray(idx.T), "dist": np.ascontiguousarray(dist.T), "w": np.ascontiguousarray(w.T),
            "sigma": sigma, "rho": rho, "init": np.ascontiguousarray(y0.T)}


def knn_classify(train, test, classes, k: int = 7, metric: str = "euclidean", ctx: Context | None = None) -> np.ndarray:
    """``class::knn(train, test, cl, k)``: for every row of ``test`` the class with the most votes among its ``k`` nearest rows of
    ``train`` (``gficf_transform_classify_host``).  Exact search; among classes that tie, the one whose first member is the
    nearer neighbour wins (``class::knn`` breaks ties at random and widens k to the points tied at the k-th distance: neither
    is reproduced).  ``classes``: one label per row of ``train``; the predictions have its dtype."""
    from . import _transform_lib

    if metric not in _lib.KNN_METRICS:
        raise ValueError(f"metric must be one of {sorted(_lib.KNN_METRICS)}")
    X, Qm = _query_pair(train, test)
    (N, d), M = X.shape, Qm.shape[0]
    classes = np.asarray(classes)
    if classes.shape != (N,):
        raise ValueError(f"classes must hold one label per row of train: {N}")
    levels, codes = np.unique(classes, return_inverse=True)
    codes = np.ascontiguousarray(codes, dtype=np.int32)
    pred = np.zeros(M, dtype=np.int32)
    ctx = ctx or default_context()
    check(_transform_lib.load().gficf_transform_classify_host(ctx.handle, _np_ptr(X), N, max(N, 1), _np_ptr(Qm), M, max(M, 1), d, int(k),
                                                              _lib.KNN_METRICS[metric], _np_ptr(codes), max(len(levels), 1), _np_ptr(pred)))
    return levels[pred]


_TRANSFORM_KW = ("n_epochs", "learning_rate", "negative_sample_rate", "repulsion_strength", "local_connectivity", "init", "query_offset",
                 "epoch_begin", "epoch_end")


def _append_predicted(embedded, new_xy):
    """The bookkeeping of embedNewCells (reference R/cellClassifier.R:83-93): trained rows NO, new rows YES, other columns NaN."""
    import pandas as pd

    emb = pd.DataFrame(embedded).copy()
    if "predicted" not in emb.columns:
        emb["predicted"] = "NO"
    df = pd.DataFrame(np.asarray(new_xy, dtype=np.float64), columns=["X", "Y"])
    for col in emb.columns[2:]:
        df[col] = np.nan
    df["predicted"] = "YES"
    out = pd.concat([emb.astype({"predicted": object}), df[list(emb.columns)]], ignore_index=True)
    out["predicted"] = pd.Categorical(out["predicted"].astype(str), categories=["NO", "YES"])
    return out


def embedNewCells(data: dict, x, nt: int = 2, seed: int = 18051982, verbose: bool = True, genes=None, ctx: Context | None = None, **kw) -> dict:
    """``embedNewCells(data, x, nt, seed, verbose, ...)`` of the reference (R/cellClassifier.R:48-95) on the device: the new
    cells are GF-ICF normalised with the trained ICF weights (:func:`gficf_with_weights`), projected into the trained PCA / LSA
    space (:func:`pca_project`) and placed into the trained plane (:func:`umap_transform`, which ``**kw`` goes to: ``n_epochs,
    learning_rate, negative_sample_rate, repulsion_strength, local_connectivity, init, query_offset, epoch_begin, epoch_end``).

    ``x``: genes x new-cells sparse count matrix whose rows are those of the matrix :func:`gficf` was given (``data["genes"]``
    selects the kept ones, standing in for the reference's match by row name), or pass ``genes``: the row of ``x`` for every
    kept gene.  ``data["embedded"]`` gets the column ``predicted`` (categorical, levels NO and YES): NO for the trained rows, YES
    for the appended new ones, whose other columns are NaN; ``data["pca"]["pred"]`` holds the new cells in PCA space.  Needs
    ``data["uwot"]`` (``runReduction(ret_model_pred=True)``); ``data["reduction"] == "tsne"`` is not provided.  ``nt`` is accepted
    for signature compatibility; ``seed`` is the reference's argument, which only its t-SNE branch uses: the sweeps take the
    model's seed."""
    import scipy.sparse as sp

    if data.get("reduction") == "tsne":
        raise NotImplementedError("embedNewCells after reduction='tsne' (the reference re-runs Rtsne) is not provided: "
                                  "run runTsne on the old and the new cells together")
    if data.get("uwot") is None:
        raise ValueError("embedNewCells needs the trained model: run runReduction(ret_model_pred=True) first")
    if data["uwot"].get("space") == "gficf":
        raise NotImplementedError("embedNewCells on a model of runReductionSparse (trained on the sparse cells, not on data['pca']; the "
                                  "reference's embedNewCells needs data$pca too) is not provided: use embedNewCellsSparse, or run runPCA and "
                                  "runReduction")
    unknown = sorted(set(kw) - set(_TRANSFORM_KW))
    if unknown:
        raise TypeError(f"embedNewCells: unknown argument(s) {unknown}")
    if data.get("pca") is None:
        raise ValueError("First run runPCA or runLSA to reduce dimensionality")
    _refuse_after_harmony(data, "embedNewCells")
    rows = np.asarray(data["genes"] if genes is None else genes, dtype=np.int64)
    if rows.shape != (len(data["w"]),):
        raise ValueError("genes must name one row of x for every kept gene (len(data['w']))")
    x = sp.csc_matrix(x)
    if len(rows) and (rows.min() < 0 or rows.max() >= x.shape[0]):
        raise ValueError(f"x has {x.shape[0]} rows: the kept genes name rows up to {int(rows.max())}")
    tsmessage(f"Embedding {x.shape[1]} new cells", verbose=verbose)
    sub = x[rows, :]
    g, kept = gficf_with_weights(sub, data["w"], ctx)
    # the rows gficf_with_weights dropped as empty come back (as empty rows): pca_project needs one per row of data["pca"]["genes"]
    g = sp.csc_matrix((g.data, kept[g.indices].astype(np.int32), g.indptr), shape=(len(rows), x.shape[1]))
    pred = pca_project(data, g, ctx)
    xy = umap_transform(pred, data["uwot"], data["pca"]["cells"], ctx=ctx, **kw)
    data["embedded"] = _append_predicted(data["embedded"], xy)
    data["pca"]["pred"] = pred
    return data


CLASSIFY_METHODS = ("PCA", "embedded", "gficf")


def classify_cells(data: dict, classes, k: int = 7, seed: int = 18051982, method: str = "PCA", ctx: Context | None = None):
    """``classify.cells(data, classes, k, seed, method)`` of the reference (R/cellClassifier.R:15-29): the new cells of
    :func:`embedNewCells` labelled by :func:`knn_classify` from the trained ones, whose labels ``classes`` are.  ``"PCA"`` searches
    ``data["pca"]["cells"]`` against ``data["pca"]["pred"]``; ``"embedded"`` the NO rows of the plane against the YES rows;
    ``"gficf"`` the sparse columns of ``data["gficf"]`` against ``data["gficf.pred"]`` of :func:`embedNewCellsSparse`
    (:func:`knn_classify_sparse`).
    Returns a DataFrame ``cell.id`` (the new cells' row labels in ``data["embedded"]``), ``pred``.  ``seed`` is accepted for
    the signature: nothing is random here."""
    import pandas as pd

    if method not in CLASSIFY_METHODS:
        raise ValueError(f"method must be one of {CLASSIFY_METHODS}")
    emb = data.get("embedded")
    if emb is None or "predicted" not in getattr(emb, "columns", ()):
        raise ValueError("Please embed first new cells!")
    new = np.asarray(emb["predicted"].astype(str) == "YES")
    if method == "gficf":
        if data.get("gficf.pred") is None:
            raise ValueError("method='gficf' needs data['gficf.pred']: embed the new cells with embedNewCellsSparse")
        pred = knn_classify_sparse(data["gficf"], data["gficf.pred"], np.asarray(classes).astype(str), k, "euclidean", ctx)
        return pd.DataFrame({"cell.id": list(emb.index[new]), "pred": pred})
    if method == "PCA":
        _refuse_after_harmony(data, "classify_cells(method='PCA')")
        train, test = data["pca"]["cells"], data["pca"]["pred"]
    else:
        xy = np.asarray(emb[["X", "Y"]], dtype=np.float64)
        train, test = xy[~new], xy[new]
    pred = knn_classify(train, test, np.asarray(classes).astype(str), k, "euclidean", ctx)
    return pd.DataFrame({"cell.id": list(emb.index[new]), "pred": pred})


# ------------------------------------------------------------------ kNN, reference-shaped
def find_nn(X, k: int, include_self: bool = True, metric: str = "manhattan", ctx: Context | None = None) -> dict:
    """The neighbour search in front of the Jaccard build, shaped like the reference's call
    ``uwot:::find_nn(X, k, include_self = T, method = "annoy", metric = dist.method)``
    (reference R/clustCells.R:57,60) — but EXACT: all N distances per row in f32, the ``k`` smallest
    (distance, index) pairs, ties broken by the smaller index.

    ``X``: N x d matrix (cells x PCA components).  Returns ``{"idx": N x k int32 (1-based), "dist":
    N x k float64}``; with ``include_self`` column 0 is the row itself (or an identical point with a
    smaller index); without it the row's own id is removed from every list (k+1 are searched).
    """
    if metric not in _lib.KNN_METRICS:
        raise ValueError(f"metric must be one of {sorted(_lib.KNN_METRICS)}")
    X = np.asfortranarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("X must be a 2-d matrix")
    N, d = X.shape
    kk = int(k) if include_self else int(k) + 1
    idx = np.zeros((kk, N), dtype=np.int32)          # C-order (kk, N) == column-major N x kk
    dist = np.zeros((kk, N), dtype=np.float64)
    ctx = ctx or default_context()
    check(_lib.load().gficf_knn_host(ctx.handle, _np_ptr(X), N, d, max(N, 1), kk, _lib.KNN_METRICS[metric],
                                     _np_ptr(idx), _np_ptr(dist)))
    return _nn_table(idx.T, dist.T, include_self)


def _nn_table(idx, dist, include_self: bool) -> dict:
    """The return of :func:`find_nn` and :func:`find_nn_sparse` from the N x kk table searched; without ``include_self`` kk was
    k + 1 and the row's own id leaves every list."""
    if not include_self:
        N, kk = idx.shape
        own = np.arange(1, N + 1, dtype=np.int32)[:, None]
        is_self = idx == own
        drop = np.where(is_self.any(axis=1), is_self.argmax(axis=1), kk - 1)   # self absent (duplicates): drop the last
        keep = np.ones_like(idx, dtype=bool)
        keep[np.arange(N), drop] = False
        idx, dist = idx[keep].reshape(N, kk - 1), dist[keep].reshape(N, kk - 1)
    return {"idx": np.ascontiguousarray(idx), "dist": np.ascontiguousarray(dist)}


# ------------------------------------------------------------------ kNN over sparse cells (libgficf_sparse_knn.so)
def find_nn_sparse_shape(G: int, N: int, k: int) -> dict:
    """The decomposition of the sparse search for ``G`` genes, ``N`` cells and ``k`` neighbours (``gficf_sparse_knn_shape``, a host
    query): ``{"tile_queries", "slices", "max_genes"}``: the query cells a workgroup holds densely in LDS (8, 4, 2 or 1, the
    fewer the more genes), the ranges the candidates are cut into when N / tile_queries workgroups would not fill the chip, and
    the largest ``G`` the search takes.  Arguments the search refuses (``G > max_genes`` among them) raise its error."""
    from . import _sparse_knn_lib

    tq, s, mg = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
    check(_sparse_knn_lib.load().gficf_sparse_knn_shape(int(G), int(N), int(k), ctypes.byref(tq), ctypes.byref(s), ctypes.byref(mg)))
    return {"tile_queries": tq.value, "slices": s.value, "max_genes": mg.value}


def _sparse_cells(M, metric, name: str = "M", min_cells: int = 1):
    """The genes x cells CSC parts of ``M`` for the sparse search, after the checks the library would only report deferred: row
    ids inside [0, G) and strictly ascending within a column, values finite as float32."""
    if metric not in _lib.KNN_METRICS:
        raise ValueError(f"metric must be one of {sorted(_lib.KNN_METRICS)}")
    if np.ndim(M) != 2:
        raise ValueError(f"{name} must be a 2-d genes x cells matrix")
    M, colptr, rowidx, x = _csc_parts(M)
    G, N = M.shape
    if G < 1 or N < min_cells:
        raise ValueError(f"{name} is {G} x {N}: the matrix needs a gene and a cell")
    if len(rowidx):
        if rowidx.min() < 0 or rowidx.max() >= G:
            raise ValueError(f"row ids must lie in [0, {G})")
        step = np.diff(rowidx) > 0
        step[colptr[1:-1][(colptr[1:-1] > 0) & (colptr[1:-1] < len(rowidx))] - 1] = True    # the seam between two columns
        if not step.all():
            raise ValueError("row ids must be strictly ascending within a column (sort_indices, sum_duplicates)")
        with np.errstate(over="ignore"):
            if not np.isfinite(x.astype(np.float32)).all():
                raise ValueError("the values must be finite as float32")
    return G, N, colptr, rowidx, x


def find_nn_sparse(M, k: int, include_self: bool = True, metric: str = "euclidean", ctx: Context | None = None) -> dict:
    """:func:`find_nn` for sparse cells: the exact neighbour search over the columns of the genes x cells matrix ``M`` (scipy
    sparse, taken as CSC; what :func:`gficf` returns as ``data["gficf"]``) without densifying it (``gficf_sparse_knn_host``,
    include/gficf_sparse_knn.h: values rounded to float32 once, pair sums in float64 over the shared genes, one rounding of the
    distance to float32).  Cosine on GF-ICF is the text-retrieval reading of this normalisation.

    Returns ``{"idx": N x k int32 (1-based), "dist": N x k float64}``, the k smallest (distance, id) pairs per cell, ties broken
    by the smaller id; with ``include_self`` column 0 is the cell itself (or an identical cell with a smaller id); without it the
    cell's own id is removed from every list (k+1 are searched).  ``idx`` is what :func:`jaccard_edges`,
    :func:`fuzzy_simplicial_set` and :func:`tsne_affinities` take.  More genes than ``find_nn_sparse_shape(...)["max_genes"]``
    raise ``GFICF_ERR_UNSUPPORTED``."""
    from . import _sparse_knn_lib

    G, N, colptr, rowidx, x = _sparse_cells(M, metric)
    k = int(k)
    if k < 1:
        raise ValueError("k must be at least 1")
    kk = k if include_self else k + 1
    idx = np.zeros((kk, N), dtype=np.int32)          # C-order (kk, N) == column-major N x kk
    dist = np.zeros((kk, N), dtype=np.float64)
    ctx = ctx or default_context()
    is64 = 1 if colptr.dtype == np.int64 else 0
    check(_sparse_knn_lib.load().gficf_sparse_knn_host(ctx.handle, G, N, _np_ptr(colptr), is64, _np_ptr(rowidx), _np_ptr(x), kk,
                                                       _lib.KNN_METRICS[metric], _np_ptr(idx), _np_ptr(dist)))
    return _nn_table(idx.T, dist.T, include_self)


def find_nn_sparse_range(M, k: int, q_begin: int, q_end: int, metric: str = "euclidean", device: int = 0) -> dict:
    """The rows ``[q_begin, q_end)`` of :func:`find_nn_sparse`'s table (``include_self=True``) through the device entry
    (``gficf_sparse_knn_device``): running ``[0, a)`` and ``[a, N)`` gives the bits of ``[0, N)``."""
    G, N, colptr, rowidx, x = _sparse_cells(M, metric)
    k, q_begin, q_end = int(k), int(q_begin), int(q_end)
    if k < 1 or not 0 <= q_begin <= q_end <= N:
        raise ValueError(f"k must be at least 1 and [q_begin, q_end) lie in [0, {N}]")
    n_q = q_end - q_begin
    ops = _umap_hip(device)
    tc, dev = ops.torch, f"cuda:{device}"
    d_cp, d_ri, d_x = (tc.from_numpy(v).to(dev) for v in (colptr.astype(np.int64), rowidx, x))
    ws = tc.empty(max(ops.sparse_knn_workspace_bytes(G, N, len(rowidx), k, n_q), 1), dtype=tc.uint8, device=dev)
    idx = tc.zeros((k, max(n_q, 1)), dtype=tc.int32, device=dev)
    dist = tc.zeros((k, max(n_q, 1)), dtype=tc.float64, device=dev)
    ops.sparse_knn(G, N, d_cp, d_ri, d_x, k, metric, q_begin, q_end, ws, idx, dist)
    ops.sparse_knn_sync(ws)
    return {"idx": np.ascontiguousarray(idx.cpu().numpy().T[:n_q]), "dist": np.ascontiguousarray(dist.cpu().numpy().T[:n_q])}


# ------------------------------------------------------------------ new sparse cells among trained ones (libgficf_sparse_query.so)
def find_nn_sparse_query_shape(G: int, N: int, M: int, k: int) -> dict:
    """The decomposition of the search of ``M`` sparse query cells among ``N`` training cells over ``G`` genes
    (``gficf_sparse_query_shape``, a host query): ``{"tile_queries", "slices", "max_genes"}``, the rule of
    :func:`find_nn_sparse_shape` for M queries against N candidates.  Arguments the search refuses raise its error."""
    from . import _sparse_query_lib

    tq, s, mg = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
    check(_sparse_query_lib.load().gficf_sparse_query_shape(int(G), int(N), int(M), int(k), ctypes.byref(tq), ctypes.byref(s), ctypes.byref(mg)))
    return {"tile_queries": tq.value, "slices": s.value, "max_genes": mg.value}


def _sparse_pair(M_train, Q, metric):
    """The CSC parts of the training cells and of the queries (which may have no columns), over the same genes."""
    t = _sparse_cells(M_train, metric, "M_train")
    q = _sparse_cells(Q, metric, "Q", min_cells=0)
    if t[0] != q[0]:
        raise ValueError(f"Q has {q[0]} rows (genes), M_train has {t[0]}")
    return t, q


def find_nn_sparse_query(M_train, Q, k: int, metric: str = "euclidean", ctx: Context | None = None) -> dict:
    """:func:`find_nn_query` for sparse cells: the ``k`` nearest columns of ``M_train`` (genes x N, scipy sparse, taken as CSC:
    ``data["gficf"]``) for every column of ``Q`` (genes x M, the same genes), exact, neither matrix densified
    (``gficf_sparse_query_host``, include/gficf_sparse_query.h: the method of :func:`find_nn_sparse` word for word, without its
    self rule).  A query equal to a training cell is at exactly 0 under euclidean and manhattan and within 2^-51 of 0 under
    cosine and correlation.  Returns ``{"idx": M x k int32, 1-based ids of training cells, "dist": M x k float64}``; a ``Q``
    without columns gives empty tables."""
    from . import _sparse_query_lib

    (G, N, tcp, tri, tx), (_, M, qcp, qri, qx) = _sparse_pair(M_train, Q, metric)
    k = int(k)
    if k < 1:
        raise ValueError("k must be at least 1")
    idx = np.zeros((k, max(M, 1)), dtype=np.int32)          # C-order (k, M) == column-major M x k
    dist = np.zeros((k, max(M, 1)), dtype=np.float64)
    ctx = ctx or default_context()
    check(_sparse_query_lib.load().gficf_sparse_query_host(
        ctx.handle, G, N, _np_ptr(tcp), 1 if tcp.dtype == np.int64 else 0, _np_ptr(tri), _np_ptr(tx), M, _np_ptr(qcp),
        1 if qcp.dtype == np.int64 else 0, _np_ptr(qri), _np_ptr(qx), k, _lib.KNN_METRICS[metric], _np_ptr(idx), _np_ptr(dist)))
    return {"idx": np.ascontiguousarray(idx.T[:M]), "dist": np.ascontiguousarray(dist.T[:M])}


def _sparse_query_enqueue(ops, t, q, k, metric, want_f32: bool):
    """Both matrices uploaded and the search enqueued: (ws, idx (k, M) int32, dist32 (k, M) float32 or None) on the device."""
    (G, N, tcp, tri, tx), (_, M, qcp, qri, qx) = t, q
    tc, dev = ops.torch, f"cuda:{ops.device}"
    d_t = [tc.from_numpy(v).to(dev) for v in (tcp.astype(np.int64), tri, tx)]
    d_q = [tc.from_numpy(v).to(dev) for v in (qcp.astype(np.int64), qri, qx)]
    ws = tc.empty(max(ops.sparse_query_workspace_bytes(G, N, len(tri), M, len(qri), k), 1), dtype=tc.uint8, device=dev)
    idx = tc.zeros((k, M), dtype=tc.int32, device=dev)
    dist32 = tc.zeros((k, M), dtype=tc.float32, device=dev) if want_f32 else None
    ops.sparse_query(G, N, *d_t, M, *d_q, k, metric, ws, idx, None, dist32)
    return ws, idx, dist32


def umap_transform_sparse(Q, model: dict, M_train, n_epochs: int | None = None, learning_rate: float | None = None,
                          negative_sample_rate: int = 5, repulsion_strength: float = 1.0, local_connectivity: float = 1.0,
                          seed: int | None = None, init="weighted", query_offset: int = 0, epoch_begin: int = 0, epoch_end: int | None = None,
                          ret_extra: bool = False, ctx: Context | None = None):
    """:func:`umap_transform` for a model of :func:`runReductionSparse` (``model["space"] == "gficf"``): the place of the columns
    of ``Q`` (genes x M sparse) in the plane of ``model``, trained on the columns of ``M_train`` (genes x N sparse,
    ``data["gficf"]``).  The same keywords, defaults and ``ret_extra`` dict as :func:`umap_transform`, and its stages on the
    device, chained through :class:`HipOps` without a host copy between them: ``sparse_query`` (float32 distances) ->
    ``transform_weights`` -> ``transform_init`` (or the given ``init``) -> ``transform_layout``.  The result for column i
    depends on that column, the model and ``query_offset + i`` only: a batch may be cut into pieces."""
    if model.get("space") != "gficf":
        raise ValueError("umap_transform_sparse needs a model of runReductionSparse (model['space'] == 'gficf'): use umap_transform")
    metric, k = model["metric"], int(model["n_neighbors"])
    t, q = _sparse_pair(M_train, Q, metric)
    N, M = t[1], q[1]
    Yt = np.ascontiguousarray(model["embedding"], dtype=np.float64)
    if Yt.shape != (N, 2):
        raise ValueError(f"model['embedding'] must be N x 2 = {N} x 2: M_train is not what the model was trained on")
    if n_epochs is None:
        n_epochs = max(1, int(round(model["n_epochs"] / 3)))
    epoch_end = int(n_epochs) if epoch_end is None else int(epoch_end)
    learning_rate = 0.25 if learning_rate is None else float(learning_rate)
    seed = int(model["seed"]) if seed is None else int(seed)
    Y0 = None
    if not (isinstance(init, str) and init == "weighted"):
        if isinstance(init, str):
            raise ValueError("init must be 'weighted' or an M x 2 array")
        Y0 = np.ascontiguousarray(init, dtype=np.float64)
        if Y0.shape != (M, 2):
            raise ValueError(f"init must be 'weighted' or an M x 2 = {M} x 2 array")
        if not np.isfinite(Y0).all():
            raise ValueError("init must be finite")
    if M == 0:
        emb = np.zeros((0, 2))
        if not ret_extra:
            return emb
        return {"embedding": emb, "idx": np.zeros((0, k), np.int32), "dist": np.zeros((0, k), np.float32), "w": np.zeros((0, k), np.float32),
                "sigma": np.zeros(0, np.float32), "rho": np.zeros(0, np.float32), "init": np.zeros((0, 2))}
    ops = _umap_hip(ctx.device if ctx is not None else 0)
    tc, dev = ops.torch, f"cuda:{ops.device}"
    sws, idx, dist = _sparse_query_enqueue(ops, t, q, k, metric, True)
    d_Yt = tc.from_numpy(Yt.astype(np.float32)).to(dev)
    w = tc.zeros((k, M), dtype=tc.float32, device=dev)
    sigma, rho = (tc.zeros(M, dtype=tc.float32, device=dev) for _ in range(2))
    wws, iws, lws = (tc.empty(max(ops.transform_workspace_bytes(s, M, k=k), 1), dtype=tc.uint8, device=dev) for s in ("weights", "init", "layout"))
    ops.transform_weights(idx, dist, N, M, k, wws, w, local_connectivity, sigma, rho)
    stages = [wws, lws]
    if Y0 is None:
        Y = tc.zeros((M, 2), dtype=tc.float32, device=dev)
        ops.transform_init(idx, w, d_Yt, N, M, k, iws, Y)
        stages.insert(1, iws)
    else:
        Y = tc.from_numpy(Y0.astype(np.float32)).to(dev)
    y0 = Y.clone() if ret_extra else None
    ops.transform_layout(idx, w, d_Yt, N, M, k, float(model["a"]), float(model["b"]), float(repulsion_strength), learning_rate,
                         int(negative_sample_rate), int(n_epochs), int(epoch_begin), epoch_end, seed, int(query_offset), Y, lws)
    ops.sparse_query_sync(sws)                                # waits for the stream; every status word after it is a read
    for ws in stages:
        ops.transform_sync(ws)
    emb = Y.cpu().numpy().astype(np.float64)
    if not ret_extra:
        return emb
    host = lambda a: np.ascontiguousarray(a.cpu().numpy().T)
    return {"embedding": emb, "idx": host(idx), "dist": host(dist), "w": host(w), "sigma": sigma.cpu().numpy(), "rho": rho.cpu().numpy(),
            "init": y0.cpu().numpy().astype(np.float64)}


def knn_classify_sparse(train, test, classes, k: int = 7, metric: str = "euclidean", ctx: Context | None = None) -> np.ndarray:
    """:func:`knn_classify` for sparse cells: for every column of ``test`` (genes x M sparse) the class with the most votes among
    its ``k`` nearest columns of ``train`` (genes x N sparse), ``sparse_query`` -> ``transform_vote`` on the device.  The label
    handling and the tie rule are :func:`knn_classify`'s.  ``classes``: one label per column of ``train``."""
    t, q = _sparse_pair(train, test, metric)
    N, M, k = t[1], q[1], int(k)
    classes = np.asarray(classes)
    if classes.shape != (N,):
        raise ValueError(f"classes must hold one label per column of train: {N}")
    if k < 1:
        raise ValueError("k must be at least 1")
    levels, codes = np.unique(classes, return_inverse=True)
    if M == 0:
        return levels[np.zeros(0, dtype=np.int64)]
    ops = _umap_hip(ctx.device if ctx is not None else 0)
    tc, dev = ops.torch, f"cuda:{ops.device}"
    sws, idx, _ = _sparse_query_enqueue(ops, t, q, k, metric, False)
    labels = tc.from_numpy(np.ascontiguousarray(codes, dtype=np.int32)).to(dev)
    pred = tc.zeros(M, dtype=tc.int32, device=dev)
    vws = tc.empty(max(ops.transform_workspace_bytes("vote", M, k=k), 1), dtype=tc.uint8, device=dev)
    ops.transform_vote(idx, labels, N, M, k, max(len(levels), 1), vws, pred)
    ops.sparse_query_sync(sws)
    ops.transform_sync(vws)
    return levels[pred.cpu().numpy()]


def embedNewCellsSparse(data: dict, x, nt: int = 2, seed: int = 18051982, verbose: bool = True, genes=None, ctx: Context | None = None,
                        **kw) -> dict:
    """:func:`embedNewCells` without the PCA step, for a model of :func:`runReductionSparse`: the new cells are GF-ICF
    normalised with the trained ICF weights (:func:`gficf_with_weights`) and placed into the trained plane by their sparse
    columns (:func:`umap_transform_sparse` against ``data["gficf"]``, which ``**kw`` goes to: the keywords of
    :func:`embedNewCells`).  ``x`` and ``genes`` are :func:`embedNewCells`'s.  ``data["embedded"]`` gets the column
    ``predicted`` as there; ``data["gficf.pred"]`` holds the new cells' GF-ICF columns (kept genes x new cells, CSC), which is
    what ``classify_cells(method="gficf")`` searches.  ``nt`` and ``seed`` are accepted for the signature."""
    import scipy.sparse as sp

    if data.get("reduction") == "tsne":
        raise NotImplementedError("embedNewCellsSparse after reduction='tsne' (the reference re-runs Rtsne) is not provided: "
                                  "run runReductionSparse(reduction='tsne') on the old and the new cells together")
    if data.get("uwot") is None:
        raise ValueError("embedNewCellsSparse needs the trained model: run runReductionSparse(ret_model_pred=True) first")
    if data["uwot"].get("space") != "gficf":
        raise ValueError("embedNewCellsSparse needs a model of runReductionSparse (trained on the sparse cells); this one was trained "
                         "on data['pca']: use embedNewCells")
    unknown = sorted(set(kw) - set(_TRANSFORM_KW))
    if unknown:
        raise TypeError(f"embedNewCellsSparse: unknown argument(s) {unknown}")
    if data.get("gficf") is None:
        raise ValueError("embedNewCellsSparse needs data['gficf']: run gficf first")
    rows = np.asarray(data["genes"] if genes is None else genes, dtype=np.int64)
    if rows.shape != (len(data["w"]),):
        raise ValueError("genes must name one row of x for every kept gene (len(data['w']))")
    x = sp.csc_matrix(x)
    if len(rows) and (rows.min() < 0 or rows.max() >= x.shape[0]):
        raise ValueError(f"x has {x.shape[0]} rows: the kept genes name rows up to {int(rows.max())}")
    tsmessage(f"Embedding {x.shape[1]} new cells (sparse)", verbose=verbose)
    sub = x[rows, :]
    g, kept = gficf_with_weights(sub, data["w"], ctx)
    # the rows gficf_with_weights dropped as empty come back (as empty rows): one per row of data["gficf"]
    g = sp.csc_matrix((g.data, kept[g.indices].astype(np.int32), g.indptr), shape=(len(rows), x.shape[1]))
    xy = umap_transform_sparse(g, data["uwot"], data["gficf"], ctx=ctx, **kw)
    data["embedded"] = _append_predicted(data["embedded"], xy)
    data["gficf.pred"] = g
    return data


def clustcells_graph(X, k: int = 15, dist_method: str = "manhattan", verbose: bool = False, ctx: Context | None = None) -> dict:
    """The graph-building lines of ``clustcells()`` (reference R/clustCells.R:57-68) as one call:
    ``neigh = find_nn(X, k+1, include_self=T)$idx; neigh[,-1]; rcpp_parallel_jaccard_coef;
    relations[relations[,3] > 0, ]``.  Returns the ``from`` / ``to`` / ``weight`` columns."""
    neigh = find_nn(X, k + 1, True, dist_method, ctx)["idx"]
    return jaccard_edges(neigh, verbose, ctx)


def phenograph(X, k: int = 15, dist_method: str = "manhattan", resolution: float = 0.8, algorithm: int = 1, n_start: int = 10,
               n_iter: int = 10, random_seed: int = 0, ctx: Context | None = None):
    """The graph build and the community detection of ``clustcells()`` (reference R/clustCells.R:57-86) chained on the
    device in one call of the C ABI (``gficf_phenograph_host``): search, ``neigh[,-1]``, Jaccard edges, ``weight > 0``,
    adjacency matrix, Louvain — one upload of ``X`` (N x d), one download of the labels.  Returns ``ClusterLabels``
    (0-based, clusters by decreasing size) with ``.modularity``, ``.n_clusters`` and ``.n_edges`` attached."""
    if dist_method not in _lib.KNN_METRICS:
        raise ValueError(f"dist_method must be one of {sorted(_lib.KNN_METRICS)}")
    X = np.asfortranarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("X must be a matrix")
    N, d = X.shape
    labels = np.zeros(max(N, 1), dtype=np.int32)
    nc, q, ne = ctypes.c_int64(0), ctypes.c_double(0.0), ctypes.c_int64(0)
    ctx = ctx or default_context()
    check(_lib.load().gficf_phenograph_host(ctx.handle, _np_ptr(X), N, d, N, int(k), _lib.KNN_METRICS[dist_method], float(resolution),
                                            int(algorithm), int(n_start), int(n_iter), int(random_seed) & 0x7FFFFFFF, _np_ptr(labels),
                                            ctypes.byref(nc), ctypes.byref(q), ctypes.byref(ne)))
    out = labels[:N].view(ClusterLabels)
    out.modularity, out.n_clusters, out.n_edges = q.value, nc.value, ne.value
    return out


COMMUNITY_ALGOS = ("louvian", "louvian 2", "louvian 3", "leiden", "slm")


def clustcells(data: dict, from_embedded: bool = False, k: int = 15, dist_method: str = "manhattan", nt: int = 2,
               community_algo: str = "louvian", store_graph: bool = True, seed: int = 180582, verbose: bool = True,
               resolution: float = 0.8, n_start: int = 10, n_iter: int = 10, ctx: Context | None = None) -> dict:
    """``clustcells(data, from.embedded, k, dist.method, nt, community.algo, store.graph, seed, verbose, resolution,
    n.start, n.iter)`` of the reference (R/clustCells.R:46-126) with every step on the device: neighbour search (:57,60,
    exact instead of Annoy), ``neigh[,-1]`` + Jaccard edges + ``weight > 0`` (:63-68), adjacency matrix (:69,80),
    community detection (:72-86, relaxed contract of ``run_modularity_clustering``), cluster signatures (:121-123).

    ``data``: dict with ``"pca": {"cells": N x d}`` (or ``"embedded"``: N x >=2 array when ``from_embedded``) and
    ``"gficf"`` (genes x cells CSC).  ``community_algo``: "louvian 2" / "louvian 3" (resolution, n_iter as given) or
    "louvian" (the reference calls igraph::cluster_louvain there: plain modularity, i.e. resolution 1) or "leiden"
    (:100-107: :func:`leiden` with ``resolution``, two iterations and ``seed``; relaxed contract of include/gficf_leiden.h);
    or "slm" (an extension: the reference's ``match.arg`` has no such choice and its "louvian 3" is algorithm 2 of the optimiser;
    :func:`slm`, algorithm 3, with ``resolution``, ``n_start``, ``n_iter`` and ``seed``, filling what "louvian 2" fills);
    the igraph algorithms "walktrap" and "fastgreedy" are third-party and not provided.  ``nt`` is accepted for
    signature compatibility (no CPU threads); ``seed`` and ``n_start`` act as in ``run_modularity_clustering``.  Returns ``data`` updated with ``community``
    (1-based like the reference), ``cluster`` (the labels as strings, ``data$embedded$cluster``), ``cluster.gene.rnk``
    (+ its column labels ``cluster.labels``) and, with ``store_graph``, ``cell.graph`` (the edge columns) and
    ``cell.adjacency``.
    """
    if community_algo not in COMMUNITY_ALGOS:
        raise ValueError(f"community_algo must be one of {COMMUNITY_ALGOS} (the igraph algorithms \"walktrap\" and \"fastgreedy\" are not provided)")
    if from_embedded:
        if data.get("embedded") is None:
            raise ValueError("First run runReduction to embed your cells")
        X = np.asarray(data["embedded"])[:, :2]
    else:
        if data.get("pca") is None:
            raise ValueError("First run runPCA or runLSA to reduce dimensionality")
        X = np.asarray(data["pca"]["cells"])
    N = X.shape[0]
    lv = (1.0, 1, 1, n_iter, 0) if community_algo == "louvian" else (resolution, 1 if community_algo == "louvian 2" else 2, n_start, n_iter, seed)
    if community_algo == "leiden":                            # the staged path either way: the fused entry is Louvain's
        edges = clustcells_graph(X, k, dist_method, verbose, ctx)
        A = jaccard_adjacency(edges, N, ctx)
        community = leiden(A, resolution, 2, seed, None, ctx)
    elif community_algo == "slm":                             # staged as well
        edges = clustcells_graph(X, k, dist_method, verbose, ctx)
        A = jaccard_adjacency(edges, N, ctx)
        community = slm(A, resolution, n_start, n_iter, seed, None, ctx)
    elif store_graph:
        edges = clustcells_graph(X, k, dist_method, verbose, ctx)
        A = jaccard_adjacency(edges, N, ctx)
        community = run_modularity_clustering(A, 1, lv[0], lv[1], lv[2], lv[3], lv[4], verbose and community_algo != "louvian", ctx)
    else:                                                     # nothing but the labels comes back: the fused entry
        community = phenograph(X, k, dist_method, lv[0], lv[1], lv[2], lv[3], lv[4], ctx)
    data["community"] = np.asarray(community, dtype=np.int32) + 1
    data["modularity"] = community.modularity
    data["cluster"] = data["community"].astype(str)
    if store_graph:
        data["cell.graph"], data["cell.adjacency"] = edges, A
    if data.get("gficf") is not None:
        data["cluster.gene.rnk"], data["cluster.labels"] = cluster_signatures(data["gficf"], data["cluster"], ctx)
    tsmessage(f"Detected Clusters: {community.n_clusters}", verbose=verbose)       # reference R/clustCells.R:125
    return data


# ------------------------------------------------------------------ Harmony: batch correction of the PCA cells
_HARMONY_OPS: dict = {}


def _harmony_ops(device: int = 0):
    """The stage object the Harmony mirrors enqueue on (one per device, made at the first call)."""
    if device not in _HARMONY_OPS:
        _HARMONY_OPS[device] = HipOps(device)
    return _HARMONY_OPS[device]


def harmony_levels(batch, N: int):
    """``batch`` (a vector, or a DataFrame or dict of vectors: V variables) as the library takes it: ``levels`` (V, N) int32 global
    level ids, ``var_start`` int32 of V + 1, and per variable its name and its labels in order of first appearance."""
    from . import _harmony_lib

    if hasattr(batch, "columns") and hasattr(batch, "__getitem__"):
        cols = [(str(c), np.asarray(batch[c])) for c in batch.columns]
    elif isinstance(batch, dict):
        cols = [(str(c), np.asarray(v)) for c, v in batch.items()]
    else:
        cols = [("batch", np.asarray(batch))]
    if not 1 <= len(cols) <= _harmony_lib.MAX_V:
        raise ValueError(f"batch must give 1 to {_harmony_lib.MAX_V} variables, not {len(cols)}")
    levels, var_start, names, labels = [], [0], [], []
    for name, col in cols:
        if col.shape != (N,):
            raise ValueError(f"batch variable {name!r} must hold one label per cell ({N}), not {col.shape}")
        ids, lab = _first_appearance_ids(col, N)
        levels.append(ids + var_start[-1])
        var_start.append(var_start[-1] + len(lab))
        names.append(name)
        labels.append(lab)
    if var_start[-1] > _harmony_lib.MAX_B:
        raise ValueError(f"batch has {var_start[-1]} levels in all: at most {_harmony_lib.MAX_B}")
    return np.ascontiguousarray(np.stack(levels), dtype=np.int32), np.asarray(var_start, dtype=np.int32), names, labels


def harmony_draws(N: int, K: int, rounds: int, seed: int = 180582):
    """The random inputs of a run, drawn in this order from ``np.random.default_rng(seed)``: K distinct cells (the start
    centroids), then one permutation of the cells per clustering round: ``(cells, perm)``, ``perm`` (rounds, N) int32."""
    rng = np.random.default_rng(seed)
    cells = rng.choice(N, K, replace=False)
    perm = np.empty((rounds, N), dtype=np.int32)
    for r in range(rounds):
        perm[r] = rng.permutation(N)
    return cells, perm


def _harmony_check_shapes(Z, levels, var_start, K=None):
    from . import _harmony_lib

    Z = np.ascontiguousarray(Z, dtype=np.float64)
    if Z.ndim != 2 or Z.shape[0] < 1 or not 1 <= Z.shape[1] <= _harmony_lib.MAX_D:
        raise ValueError(f"the cells must be an N x d matrix with 1 <= d <= {_harmony_lib.MAX_D}")
    if not np.isfinite(Z).all():
        raise ValueError("the cells hold a value that is not finite")
    N = Z.shape[0]
    if levels is not None:
        levels = np.ascontiguousarray(levels, dtype=np.int32)
        var_start = np.ascontiguousarray(var_start, dtype=np.int32)
        if levels.ndim != 2 or levels.shape[1] != N or not 1 <= levels.shape[0] <= _harmony_lib.MAX_V:
            raise ValueError(f"levels must be V x N with 1 <= V <= {_harmony_lib.MAX_V}")
        V = levels.shape[0]
        if var_start.shape != (V + 1,) or var_start[0] != 0 or (np.diff(var_start) < 1).any() or var_start[-1] > _harmony_lib.MAX_B:
            raise ValueError(f"var_start must rise from 0 by at least 1 a variable to B <= {_harmony_lib.MAX_B}")
        if ((levels < var_start[:-1, None]) | (levels >= var_start[1:, None])).any():
            raise ValueError("a level id lies outside its variable's range")
    if K is not None and not 1 <= K <= min(N, _harmony_lib.MAX_K):
        raise ValueError(f"the number of clusters must be in [1, min(N, {_harmony_lib.MAX_K})], not {K}")
    return Z, levels, var_start


def _harmony_per_level(x, var_start, what, lo=0.0):
    """A scalar, one value per variable or one per level, as one float64 per level."""
    B, V = int(var_start[-1]), len(var_start) - 1
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    if x.shape == (1,):
        x = np.full(B, x[0])
    elif x.shape == (V,) and V != B:
        x = np.repeat(x, np.diff(var_start))
    elif x.shape != (B,):
        raise ValueError(f"{what} must be a scalar, one value per variable ({V}) or one per level ({B})")
    if not np.isfinite(x).all() or (x < lo).any():
        raise ValueError(f"{what} must be finite and at least {lo}")
    return np.ascontiguousarray(x)


class _HarmonyState:
    """The device tensors of a Harmony problem, and the stages on them."""

    def __init__(self, Z, levels, var_start, K, device: int = 0):
        self.ops = _harmony_ops(device)
        tc = self.ops.torch
        self.tc, self.dev = tc, tc.device("cuda", device)
        self.N, self.d = Z.shape
        self.K = int(K)
        if levels is None:
            levels, var_start = np.zeros((1, self.N), dtype=np.int32), np.array([0, 1], dtype=np.int32)
        self.V, self.B, self.var_start = levels.shape[0], int(var_start[-1]), var_start
        self.Z, self.levels = self.up(Z), self.up(levels)
        self.ws = tc.zeros(self.ops.harmony_workspace_bytes(self.N, self.d, self.K, self.V, self.B), dtype=tc.uint8, device=self.dev)

    def up(self, a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        return self.tc.from_numpy(a if a.flags.writeable else a.copy()).to(self.dev)

    def f64(self, *shape):
        return self.tc.zeros(shape, dtype=self.tc.float64, device=self.dev)

    def sync(self):
        return self.ops.harmony_sync(self.ws)


def harmony_normalise(Z):
    """Stage 1 of include/gficf_harmony.h alone: the rows of ``Z`` scaled to unit length (a zero row stays zero)."""
    Z, _, _ = _harmony_check_shapes(Z, None, None)
    s = _HarmonyState(Z, None, None, 1)
    Zc = s.f64(s.N, s.d)
    s.ops.harmony_normalise(s.Z, Zc, s.ws)
    s.sync()
    return Zc.cpu().numpy()


def harmony_start(Zc, Y0, init_iter: int = 10) -> dict:
    """Stage 2 alone: ``init_iter`` hard Lloyd iterations under cosine from the centroids ``Y0``: ``{"Y", "labels"}``."""
    Y0 = np.ascontiguousarray(Y0, dtype=np.float64)
    Zc, _, _ = _harmony_check_shapes(Zc, None, None, K=Y0.shape[0] if Y0.ndim == 2 else 0)
    if Y0.ndim != 2 or Y0.shape[1] != Zc.shape[1]:
        raise ValueError("Y0 must be K x d")
    if init_iter < 0:
        raise ValueError("init_iter must not be negative")
    s = _HarmonyState(Zc, None, None, Y0.shape[0])
    Y, lab = s.f64(s.K, s.d), s.tc.zeros(s.N, dtype=s.tc.int32, device=s.dev)
    s.ops.harmony_start(s.up(Zc), s.up(Y0), int(init_iter), Y, lab, s.ws)
    s.sync()
    return {"Y": Y.cpu().numpy(), "labels": lab.cpu().numpy()}


def _harmony_stage_args(Zc, levels, var_start, Y, sigma, R=None, O=None, E=None, theta=None):
    """The arguments the stage mirrors share, checked before a device is touched."""
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    Zc, levels, var_start = _harmony_check_shapes(Zc, levels, var_start, K=Y.shape[0] if Y.ndim == 2 else 0)
    if levels is None:
        raise ValueError("levels and var_start are needed")
    if Y.ndim != 2 or Y.shape[1] != Zc.shape[1]:
        raise ValueError("Y must be K x d")
    if not (np.isfinite(sigma) and sigma > 0):
        raise ValueError("sigma must be positive and finite")
    K, N, B = Y.shape[0], Zc.shape[0], int(var_start[-1])
    roe = []
    for a, shape, name in ((R, (K, N), "R"), (O, (K, B), "O"), (E, (K, B), "E")):
        if a is not None:
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.shape != shape:
                raise ValueError(f"{name} must be {shape[0]} x {shape[1]}")
        roe.append(a)
    if theta is not None:
        theta = _harmony_per_level(theta, var_start, "theta")
    return Zc, levels, var_start, Y, roe, theta


def harmony_assign(Zc, levels, var_start, Y, sigma: float = 0.1) -> dict:
    """Stage 3 alone: ``{"R", "O", "E"}`` of the centroids ``Y`` without penalty."""
    Zc, levels, var_start, Y, _, _ = _harmony_stage_args(Zc, levels, var_start, Y, sigma)
    s = _HarmonyState(Zc, levels, var_start, Y.shape[0])
    R, O, E = s.f64(s.K, s.N), s.f64(s.K, s.B), s.f64(s.K, s.B)
    s.ops.harmony_assign(s.Z, s.levels, s.var_start, s.up(Y), sigma, R, O, E, s.ws)
    s.sync()
    return {"R": R.cpu().numpy(), "O": O.cpu().numpy(), "E": E.cpu().numpy()}


def harmony_round(Zc, levels, var_start, Y, R, O, E, theta, sigma, perm, n_blocks: int) -> dict:
    """Stage 4 alone: one clustering round over the ``n_blocks`` blocks of the permutation ``perm``: ``{"R", "O", "E", "Y"}``."""
    Zc, levels, var_start, Y, (R, O, E), theta = _harmony_stage_args(Zc, levels, var_start, Y, sigma, R, O, E, theta)
    perm = np.ascontiguousarray(perm, dtype=np.int32)
    if perm.shape != (Zc.shape[0],) or not np.array_equal(np.sort(perm), np.arange(Zc.shape[0])):
        raise ValueError("perm must be a permutation of the cells")
    if n_blocks < 1:
        raise ValueError("n_blocks must be at least 1")
    s = _HarmonyState(Zc, levels, var_start, Y.shape[0])
    Rd, Od, Ed, Yd = s.up(R), s.up(O), s.up(E), s.up(Y)
    s.ops.harmony_round(s.Z, s.levels, s.var_start, s.up(theta), sigma, s.up(perm), int(n_blocks), Rd, Od, Ed, Yd, s.ws)
    s.sync()
    return {"R": Rd.cpu().numpy(), "O": Od.cpu().numpy(), "E": Ed.cpu().numpy(), "Y": Yd.cpu().numpy()}


def harmony_objective(Zc, levels, var_start, Y, R, O, E, theta, sigma: float = 0.1) -> float:
    """Stage 5 alone: the objective of (Y, R, O, E)."""
    Zc, levels, var_start, Y, (R, O, E), theta = _harmony_stage_args(Zc, levels, var_start, Y, sigma, R, O, E, theta)
    s = _HarmonyState(Zc, levels, var_start, Y.shape[0])
    obj = s.f64(1)
    s.ops.harmony_objective(s.Z, s.levels, s.var_start, s.up(Y), s.up(R), s.up(O), s.up(E), s.up(theta), sigma, obj, s.ws)
    s.sync()
    return float(obj.cpu()[0])


def harmony_correct(Z, levels, var_start, R, lamb=1.0) -> dict:
    """Stage 6 alone: ``{"Z": the corrected cells, "W": (K, B + 1, d) ridge coefficients, "flat_clusters"}``."""
    R = np.ascontiguousarray(R, dtype=np.float64)
    Z, levels, var_start = _harmony_check_shapes(Z, levels, var_start, K=R.shape[0] if R.ndim == 2 else 0)
    if levels is None:
        raise ValueError("levels and var_start are needed")
    if R.ndim != 2 or R.shape[1] != Z.shape[0]:
        raise ValueError("R must be K x N")
    lamb = _harmony_per_level(lamb, var_start, "lamb")
    s = _HarmonyState(Z, levels, var_start, R.shape[0])
    Zcorr, W = s.f64(s.N, s.d), s.f64(s.K, s.B + 1, s.d)
    s.ops.harmony_correct(s.Z, s.levels, s.var_start, s.up(R), s.up(lamb), Zcorr, s.ws, W)
    info = s.sync()
    return {"Z": Zcorr.cpu().numpy(), "W": W.cpu().numpy(), "flat_clusters": info["flat_clusters"]}


def _harmony_setup(X, batch, theta, lamb, sigma, nclust, tau, block_size, max_iter_harmony, max_iter_kmeans, epsilon_cluster, epsilon_harmony,
                   init_iter):
    """The argument checks of :func:`harmony_matrix`, and what it derives on the host."""
    X, _, _ = _harmony_check_shapes(X, None, None)
    N = X.shape[0]
    levels, var_start, names, labels = harmony_levels(batch, N)
    K = min(int(round(N / 30.0)), 100) if nclust is None else int(nclust)
    K = max(K, 1) if nclust is None else K
    _harmony_check_shapes(X, levels, var_start, K=K)
    if not (np.isfinite(sigma) and sigma > 0):
        raise ValueError("sigma must be positive and finite")
    if not 0 < block_size <= 1:
        raise ValueError("block_size must be in (0, 1]")
    if min(max_iter_harmony, max_iter_kmeans, init_iter) < 0:
        raise ValueError("the iteration limits must not be negative")
    if tau < 0:
        raise ValueError("tau must not be negative")
    theta = _harmony_per_level(theta, var_start, "theta")
    lamb = _harmony_per_level(lamb, var_start, "lamb")
    if tau > 0:
        counts = np.stack([(levels == b).sum() for b in range(int(var_start[-1]))]).astype(np.float64)
        theta = theta * (1.0 - np.exp(-(counts / (K * tau)) ** 2))
    return dict(X=X, levels=levels, var_start=var_start, names=names, labels=labels, K=K, theta=theta, lamb=lamb, sigma=float(sigma),
                n_blocks=int(np.ceil(1.0 / block_size)), max_iter_harmony=int(max_iter_harmony), max_iter_kmeans=int(max_iter_kmeans),
                epsilon_cluster=float(epsilon_cluster), epsilon_harmony=float(epsilon_harmony), init_iter=int(init_iter))


def harmony_matrix(X, batch, theta=2.0, lamb=1.0, sigma: float = 0.1, nclust: int | None = None, tau: float = 0.0, block_size: float = 0.05,
                   max_iter_harmony: int = 10, max_iter_kmeans: int = 20, epsilon_cluster: float = 1e-5, epsilon_harmony: float = 1e-4,
                   seed: int = 180582, init_iter: int = 10) -> dict:
    """Harmony (Korsunsky et al. 2019) of the N x d cells ``X`` for the batch variable(s) ``batch``, on the device: the chain of
    include/gficf_harmony.h (``gficf_harmony_device``).  Returns ``Z`` (the corrected cells), ``R`` (K x N soft assignments), ``Y``
    (K x d centroids), ``objective`` (the last objective of every outer iteration), ``objective_rounds`` (every round's, the
    start's first), ``iter_rounds``, ``iterations``, ``rounds``, ``converged``, ``levels`` (per variable, its labels in order of
    first appearance), ``flat_clusters`` (clusters the last correction left out) and ``last_change`` (the last relative drop).

    ``nclust=None``: ``min(round(N / 30), 100)``, at least 1.  ``theta`` and ``lamb``: a scalar, or one value per variable (or per
    level).  ``tau > 0`` scales ``theta[b]`` by ``1 - exp(-(N_b / (K tau))^2)``.  The random inputs are those of
    :func:`harmony_draws` with ``seed``: the start centroids are the drawn cells, normalised."""
    p = _harmony_setup(X, batch, theta, lamb, sigma, nclust, tau, block_size, max_iter_harmony, max_iter_kmeans, epsilon_cluster, epsilon_harmony,
                       init_iter)
    X, K = p["X"], p["K"]
    N = X.shape[0]
    cells, perm = harmony_draws(N, K, p["max_iter_harmony"] * p["max_iter_kmeans"], seed)
    s = _HarmonyState(X, p["levels"], p["var_start"], K)
    Y0 = s.up(X[cells])
    s.ops.harmony_normalise(Y0, Y0, s.ws)
    Zcorr, Zc, R, Y, O, E = s.f64(s.N, s.d), s.f64(s.N, s.d), s.f64(K, s.N), s.f64(K, s.d), s.f64(K, s.B), s.f64(K, s.B)
    permd = s.up(perm) if perm.shape[0] else s.tc.zeros((0, N), dtype=s.tc.int32, device=s.dev)
    out = s.ops.harmony(s.Z, s.levels, s.var_start, s.up(p["theta"]), s.up(p["lamb"]), p["sigma"], Y0, permd, p["init_iter"], p["max_iter_harmony"],
                        p["max_iter_kmeans"], p["n_blocks"], p["epsilon_cluster"], p["epsilon_harmony"], Zcorr, Zc, R, Y, O, E, s.ws)
    info = s.sync()
    ends = np.cumsum(out["iter_rounds"])
    h = out["objective"][ends]
    last = float((h[-2] - h[-1]) / abs(h[-2])) if len(h) >= 2 else float("nan")
    return {"Z": Zcorr.cpu().numpy(), "R": R.cpu().numpy(), "Y": Y.cpu().numpy(), "objective": h, "objective_rounds": out["objective"],
            "iter_rounds": out["iter_rounds"], "iterations": out["iterations"], "rounds": out["rounds"], "converged": out["converged"],
            "levels": dict(zip(p["names"], p["labels"])), "flat_clusters": info["flat_clusters"], "zero_rows": info["zero_rows"],
            "last_change": last, "nclust": K, "theta": p["theta"], "lamb": p["lamb"], "n_blocks": p["n_blocks"]}


def runHarmony(data: dict, batch, theta=2.0, lamb=1.0, sigma: float = 0.1, nclust: int | None = None, tau: float = 0.0, block_size: float = 0.05,
               max_iter_harmony: int = 10, max_iter_kmeans: int = 20, epsilon_cluster: float = 1e-5, epsilon_harmony: float = 1e-4,
               seed: int = 180582) -> dict:
    """Harmony batch correction of ``data["pca"]["cells"]`` between :func:`runPCA` and :func:`runReduction` / :func:`clustcells`
    (the reference's later releases add ``runHarmony`` at this place): see :func:`harmony_matrix`.  ``data["pca"]["cells"]`` becomes
    the corrected matrix, ``data["pca"]["cells_uncorrected"]`` keeps the original (a second call starts from it again) and
    ``data["pca"]["harmony"]`` holds the parameters, ``iterations``, ``objective`` and ``converged``.  New cells are not corrected:
    :func:`embedNewCells` and ``classify_cells(method="PCA")`` refuse a ``data`` that carries ``data["pca"]["harmony"]``."""
    if data.get("pca") is None:
        raise ValueError("First run runPCA or runLSA to reduce dimensionality")
    pca = data["pca"]
    orig = np.asarray(pca["cells_uncorrected"] if pca.get("cells_uncorrected") is not None else pca["cells"], dtype=np.float64)
    r = harmony_matrix(orig, batch, theta, lamb, sigma, nclust, tau, block_size, max_iter_harmony, max_iter_kmeans, epsilon_cluster, epsilon_harmony, seed)
    if not r["converged"]:
        warnings.warn(f"runHarmony did not converge in {max_iter_harmony} iterations: the last relative change of the objective was "
                      f"{r['last_change']:.3g} (epsilon_harmony = {epsilon_harmony:g})")
    pca["cells_uncorrected"] = orig
    pca["cells"] = r["Z"]
    pca["harmony"] = {"theta": r["theta"], "lamb": r["lamb"], "sigma": float(sigma), "nclust": r["nclust"], "tau": float(tau),
                      "block_size": float(block_size), "max_iter_harmony": int(max_iter_harmony), "max_iter_kmeans": int(max_iter_kmeans),
                      "epsilon_cluster": float(epsilon_cluster), "epsilon_harmony": float(epsilon_harmony), "seed": int(seed),
                      "levels": r["levels"], "iterations": r["iterations"], "rounds": r["rounds"], "objective": r["objective"],
                      "converged": r["converged"], "flat_clusters": r["flat_clusters"]}
    return data


def _refuse_after_harmony(data: dict, what: str):
    if isinstance(data.get("pca"), dict) and data["pca"].get("harmony") is not None:
        raise NotImplementedError(f"{what} after runHarmony is not provided: new cells are not batch corrected, so they cannot be placed among "
                                  "the corrected data['pca']['cells']")


# ----------------------------------------------------------- device-resident stage ops
def genes_words(G: int) -> int:
    """float64 elements of the opaque per-gene table buffer (gficf_csc_genes_bytes)."""
    return int(_lib.load().gficf_csc_genes_bytes(int(G)) + 7) // 8


def _tptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError("expected a CUDA (HIP) tensor")
    if not t.is_contiguous():
        raise ValueError("expected a contiguous tensor")
    return ctypes.c_void_p(t.data_ptr())


class HipOps:
    """Pipeline stages of the hot path on device-resident torch tensors.

    Work is enqueued on torch's current stream of the context's device; nothing
    synchronises except :meth:`sync`.
    """

    def __init__(self, device: int = 0):
        import torch

        self.torch = torch
        self.device = int(device)
        self.ctx = Context(self.device)
        self.L = _lib.load()
        self._raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)

    def current_stream(self) -> int:
        """torch's current stream of this device as a raw hipStream_t (no Stream object built: this sits on every enqueue)."""
        raw = self._raw_stream
        return raw(self.device) if raw is not None else self.torch.cuda.current_stream(self.device).cuda_stream

    def _bind(self):
        self.ctx.set_stream(self.current_stream())
        return self.ctx.handle

    def sync(self):
        self._bind()
        self.ctx.sync()

    def set_jaccard_distinct(self, assume_distinct: bool):
        """See :meth:`Context.set_jaccard_distinct` (the option belongs to the context these ops enqueue on)."""
        self.ctx.set_jaccard_distinct(assume_distinct)

    def set_jaccard_direct_max_edges(self, max_edges: int):
        """See :meth:`Context.set_jaccard_direct_max_edges`."""
        self.ctx.set_jaccard_direct_max_edges(max_edges)

    def jaccard_one_launch(self, N: int, k: int) -> bool:
        """Would :meth:`jaccard` build an N x k problem in ONE launch, as the context is set up now?"""
        return bool(self.L.gficf_jaccard_one_launch(self.ctx.handle, int(N), int(k)))

    # -- Jaccard
    @staticmethod
    def kpad(k: int) -> int:
        kp = _lib.load().gficf_jaccard_kpad(int(k))
        if kp < 0:
            raise GficfError(6, f"k = {k} outside [0, {_lib.JACCARD_MAX_K_EXACT}]")
        return kp

    @staticmethod
    def row_words(N_total: int, k: int) -> int:
        """Row pitch (int32 words) of the table of an N_total-cell data set: kpad(k), or half of it where the
        library stores the rows compactly (fewer than 2^17 cells).  Tables are (N, row_words) int32."""
        rw = _lib.load().gficf_jaccard_row_words(int(N_total), int(k))
        if rw < 0:
            raise GficfError(6, f"k = {k} outside [0, {_lib.JACCARD_MAX_K_EXACT}] or N_total = {N_total} beyond int32 ids")
        return rw

    def jaccard_ingest(self, idx_cm, n_rows: int, k: int, N_total: int, table_rows):
        """idx_cm: (k, ld) int32/float64 tensor == column-major n_rows x k.  table_rows: (n_rows, row_words) int32."""
        tc = self.torch
        is_f64 = 1 if idx_cm.dtype == tc.float64 else 0
        if not is_f64 and idx_cm.dtype != tc.int32:
            raise ValueError("idx must be int32 or float64")
        ld = idx_cm.shape[1] if idx_cm.dim() == 2 else n_rows
        check(self.L.gficf_jaccard_ingest_device(self._bind(), _tptr(idx_cm), is_f64, n_rows, k, ld, N_total,
                                                 _tptr(table_rows)))

    @staticmethod
    def packed_words(N_total: int, k: int) -> int:
        return int(_lib.load().gficf_jaccard_packed_words(int(N_total), int(k)))

    def jaccard_pack_rows(self, table_rows, n_rows: int, k: int, N_total: int, packed):
        """table_rows (n_rows, row_words) int32 -> packed (n_rows, packed_words) int32 (transport form)."""
        check(self.L.gficf_jaccard_pack_rows_device(self._bind(), _tptr(table_rows), n_rows, k, N_total, _tptr(packed)))

    def jaccard_unpack_rows(self, packed, n_rows: int, k: int, N_total: int, table_rows):
        check(self.L.gficf_jaccard_unpack_rows_device(self._bind(), _tptr(packed), n_rows, k, N_total, _tptr(table_rows)))

    def jaccard_edges(self, table, N: int, k: int, cell_begin: int, cell_end: int, out3, u=None):
        """table: (N, row_words) int32.  out3: (3, (cell_end-cell_begin)*k) float64 — src, dst, weight rows."""
        n = (cell_end - cell_begin) * k
        if out3.shape != (3, n) or out3.dtype != self.torch.float64:
            raise ValueError(f"out3 must be float64 of shape (3, {n})")
        base = out3.data_ptr()
        check(self.L.gficf_jaccard_edges_device(self._bind(), _tptr(table), N, k, cell_begin, cell_end,
                                                ctypes.c_void_p(base), ctypes.c_void_p(base + 8 * n),
                                                ctypes.c_void_p(base + 16 * n), _tptr(u)))

    # -- the sharded build on local ids (csrc/halo.hip; gficf_amd.dist.JaccardHaloShard)
    def halo_workspace_bytes(self, N_total: int, P: int) -> int:
        return int(self.L.gficf_jaccard_halo_workspace_bytes(int(N_total), int(P)))

    def halo_ingest_peer(self, idx_cm, n_local, k, N_total, cell_begin, P, rows_per_rank, cap, ws, req_out, owner_blocks, table, l2g):
        """The whole table of the sub-problem in one launch behind the plan, with nothing exchanged: ``owner_blocks[o]`` is owner o's
        (k, ld_o) int32 block of global ids in memory this device can read (its own, or a peer's through the peer mapping)."""
        if len(owner_blocks) != P:
            raise ValueError("one block per owner")
        ptrs = (ctypes.c_void_p * P)(*[(t.data_ptr() if t is not None and t.numel() else None) for t in owner_blocks])
        lds = (ctypes.c_int64 * P)(*[(int(t.shape[1]) if t is not None and t.dim() == 2 and t.numel() else 0) for t in owner_blocks])
        ld = idx_cm.shape[1] if idx_cm.dim() == 2 else n_local
        check(self.L.gficf_jaccard_halo_ingest_peer_device(self._bind(), _tptr(idx_cm), n_local, k, ld, N_total, cell_begin, P, rows_per_rank, cap,
                                                           _tptr(ws), _tptr(req_out), ptrs, lds, _tptr(table), _tptr(l2g)))

    def halo_plan(self, idx_cm, n_local, k, N_total, cell_begin, P, rows_per_rank, cap, ws, req_out):
        """idx_cm: (k, ld) int32, the block's global ids.  Fills req_out (P * cap int32: ids asked of every owner, 0 = empty)."""
        if idx_cm.dtype != self.torch.int32:
            raise ValueError("the halo exchange carries int32 ids")
        ld = idx_cm.shape[1] if idx_cm.dim() == 2 else n_local
        check(self.L.gficf_jaccard_halo_plan_device(self._bind(), _tptr(idx_cm), n_local, k, ld, N_total, cell_begin, P, rows_per_rank, cap,
                                                    _tptr(ws), _tptr(req_out)))

    def halo_serve(self, idx_cm, n_local, k, cell_begin, req_in, rows_out):
        ld = idx_cm.shape[1] if idx_cm.dim() == 2 else n_local
        check(self.L.gficf_jaccard_halo_serve_device(self._bind(), _tptr(idx_cm), n_local, k, ld, cell_begin, _tptr(req_in), int(req_in.numel()),
                                                     _tptr(rows_out)))

    def halo_relabel(self, idx_cm, n_local, k, N_total, cell_begin, P, rows_per_rank, cap, ws, req_out, rows_in, idx_ext, l2g):
        ld = idx_cm.shape[1] if idx_cm.dim() == 2 else n_local
        check(self.L.gficf_jaccard_halo_relabel_device(self._bind(), _tptr(idx_cm), n_local, k, ld, N_total, cell_begin, P, rows_per_rank, cap,
                                                       _tptr(ws), _tptr(req_out), _tptr(rows_in), _tptr(idx_ext), _tptr(l2g)))

    def halo_serve_ingest(self, idx_cm, n_local, k, N_total, cell_begin, P, rows_per_rank, cap, ws, req_out, req_in, rows_out, table, l2g) -> bool:
        """Between the two exchanges, ONE launch (k <= 64): the rows asked of this rank (``req_in`` -> ``rows_out``) and the table
        rows of the own cells (they need the plan, not the replies).  False: k > 64, nothing enqueued (run the unfused calls)."""
        if k > 64:
            return False
        ld = idx_cm.shape[1] if idx_cm.dim() == 2 else n_local
        check(self.L.gficf_jaccard_halo_serve_ingest_device(self._bind(), _tptr(idx_cm), n_local, k, ld, N_total, cell_begin, P, rows_per_rank, cap,
                                                            _tptr(ws), _tptr(req_out), _tptr(req_in), int(req_in.numel()), _tptr(rows_out),
                                                            _tptr(table), _tptr(l2g)))
        return True

    def halo_ingest_slots(self, idx_cm, n_local, k, N_total, cell_begin, P, rows_per_rank, cap, ws, req_out, rows_in, table, l2g):
        """Behind the second exchange: the table rows of the halo slots in use, from the replies (k <= 64)."""
        ld = idx_cm.shape[1] if idx_cm.dim() == 2 else n_local
        check(self.L.gficf_jaccard_halo_ingest_slots_device(self._bind(), _tptr(idx_cm), n_local, k, ld, N_total, cell_begin, P, rows_per_rank, cap,
                                                            _tptr(ws), _tptr(req_out), _tptr(rows_in), _tptr(table), _tptr(l2g)))

    def jaccard_ingest_local(self, idx_ext, n_ext, k, table):
        """idx_ext: (k, n_ext) int32 local ids (0 = no id).  table: (n_ext, row_words(n_ext, k)) int32."""
        check(self.L.gficf_jaccard_ingest_local_device(self._bind(), _tptr(idx_ext), n_ext, k, n_ext, _tptr(table)))

    def jaccard_edges_mapped(self, table, n_ext, k, n_cells, src_offset, l2g, out3, u=None):
        """Edges of the first n_cells rows of a local-id table; column 1 = src_offset + cell + 1, column 2 = l2g[local - 1]."""
        n = n_cells * k
        if out3.shape != (3, n) or out3.dtype != self.torch.float64:
            raise ValueError(f"out3 must be float64 of shape (3, {n})")
        base = out3.data_ptr()
        check(self.L.gficf_jaccard_edges_mapped_device(self._bind(), _tptr(table), n_ext, k, n_cells, src_offset, _tptr(l2g),
                                                       ctypes.c_void_p(base), ctypes.c_void_p(base + 8 * n), ctypes.c_void_p(base + 16 * n),
                                                       _tptr(u)))

    def jaccard_edges_filtered(self, table, N: int, k: int, cell_begin: int, cell_end: int, u_ws, cell_ptr, out3):
        """Edges with u > 0 only, in order (reference R/clustCells.R:66).  u_ws: int16 workspace of n*k;
        cell_ptr: int64 (n+1); out3: (3, n*k) float64 capacity — rows from / to / weight, first cell_ptr[n] valid."""
        n = (cell_end - cell_begin) * k
        base = out3.data_ptr()
        check(self.L.gficf_jaccard_edges_filtered_device(self._bind(), _tptr(table), N, k, cell_begin, cell_end,
                                                         _tptr(u_ws), _tptr(cell_ptr), ctypes.c_void_p(base),
                                                         ctypes.c_void_p(base + 8 * n), ctypes.c_void_p(base + 16 * n)))

    def adjacency_workspace_bytes(self, N: int, edge_capacity: int) -> int:
        return int(self.L.gficf_adjacency_workspace_bytes(int(N), int(edge_capacity)))

    def adjacency(self, N: int, edge_capacity: int, n_edges_dev, out3, ws, indptr, indices, x, grouped_by_source: bool = False):
        """out3: the (3, edge_capacity) float64 buffer of jaccard_edges_filtered (rows from / to / weight);
        n_edges_dev: int64 device scalar (a 1-element view, e.g. cell_ptr[n:n+1]) or None = all edge_capacity rows.
        grouped_by_source: the caller knows that the edges of one source cell lie together (what jaccard_edges_filtered writes):
        no check, no stream synchronisation inside the call; False = any edge list."""
        base = out3.data_ptr()
        check(self.L.gficf_adjacency_device(self._bind(), N, edge_capacity, _tptr(n_edges_dev), ctypes.c_void_p(base),
                                            ctypes.c_void_p(base + 8 * edge_capacity), ctypes.c_void_p(base + 16 * edge_capacity),
                                            1 if grouped_by_source else 0, _tptr(ws), int(ws.numel()), _tptr(indptr), _tptr(indices), _tptr(x)))

    def jaccard(self, idx_cm, N: int, k: int, table_ws, rmat3, u=None):
        """Single-GPU ingest + edges.  rmat3: (3, N*k) float64 == the (N*k) x 3 R matrix."""
        tc = self.torch
        is_f64 = 1 if idx_cm.dtype == tc.float64 else 0
        ld = idx_cm.shape[1] if idx_cm.dim() == 2 else N
        check(self.L.gficf_jaccard_device(self._bind(), _tptr(idx_cm), is_f64, N, k, ld, _tptr(table_ws),
                                          _tptr(rmat3), _tptr(u)))

    def jaccard_prepared(self, idx_cm, N: int, k: int, table_ws, rmat3, u=None):
        """The same call with every argument converted ONCE: returns ``run()``, one call into the library per invocation
        (gficf_jaccard_device: for a small problem under gficf_ctx_set_jaccard_distinct ONE launch, otherwise ingest + edges), on
        torch's current stream at the time of the invocation.  For steps of a few microseconds, where building the ctypes
        arguments of :meth:`jaccard` costs as much as the kernels (BASELINE configs 1 - 3).  The tensors are kept alive by the
        callable and must not be resized."""
        tc = self.torch
        is_f64 = 1 if idx_cm.dtype == tc.float64 else 0
        if not is_f64 and idx_cm.dtype != tc.int32:
            raise ValueError("idx must be int32 or float64")
        ld = idx_cm.shape[1] if idx_cm.dim() == 2 else N
        if rmat3.shape != (3, N * k) or rmat3.dtype != tc.float64:
            raise ValueError(f"rmat3 must be float64 of shape (3, {N * k})")
        fn, ctx, cur = self.L.gficf_jaccard_device, self.ctx, self.current_stream
        args = (ctx.handle, _tptr(idx_cm), is_f64, int(N), int(k), int(ld), _tptr(table_ws), _tptr(rmat3), _tptr(u))

        def run():
            s = cur()
            if s != ctx._stream:
                ctx.set_stream(s)
            rc = fn(*args)
            if rc:
                check(rc)

        run.keep = (idx_cm, table_ws, rmat3, u)
        return run

    # -- exact kNN (next row N2)
    @staticmethod
    def knn_dpad(d: int) -> int:
        dp = _lib.load().gficf_knn_dpad(int(d))
        if dp < 0:
            raise GficfError(6, f"d = {d} outside [0, 128]")
        return dp

    def knn_prepare(self, X_cm, n_rows: int, d: int, metric: str, point_rows):
        """X_cm: (d, ld) float64/float32 tensor == column-major n_rows x d block of the R matrix.
        point_rows: (n_rows, dpad) float32."""
        tc = self.torch
        is_f64 = 1 if X_cm.dtype == tc.float64 else 0
        if not is_f64 and X_cm.dtype != tc.float32:
            raise ValueError("X must be float64 or float32")
        ld = X_cm.shape[1] if X_cm.dim() == 2 else n_rows
        check(self.L.gficf_knn_prepare_device(self._bind(), _tptr(X_cm), is_f64, n_rows, d, ld, _lib.KNN_METRICS[metric],
                                              _tptr(point_rows)))

    def knn_workspace_bytes(self, n_queries: int, N: int, k: int) -> int:
        return int(self.L.gficf_knn_workspace_bytes(self.ctx.handle, n_queries, N, k))

    def knn_search(self, points, N: int, d: int, k: int, metric: str, q_begin: int, q_end: int, ws, idx_cm, dist_cm=None):
        """points: (N, dpad) float32.  idx_cm: (k, ld) int32 == column-major (q_end-q_begin) x k, 1-based ids;
        dist_cm: same shape float32 or None.  ws: uint8 scratch of knn_workspace_bytes()."""
        ld = idx_cm.shape[1] if idx_cm.dim() == 2 else q_end - q_begin
        check(self.L.gficf_knn_search_device(self._bind(), _tptr(points), N, d, k, _lib.KNN_METRICS[metric], q_begin, q_end,
                                             _tptr(ws), int(ws.numel()), _tptr(idx_cm), _tptr(dist_cm), ld))

    def knn_pivot_order(self, points, N: int, d: int, metric: str, ws, order):
        """order (N int32): order[p] = 0-based row of the point at position p of the pruned search's (coarse, fine) pivot order —
        a cell numbering with locality.  ws: uint8 scratch of knn_workspace_bytes(N, N, 1)."""
        check(self.L.gficf_knn_pivot_order_device(self._bind(), _tptr(points), N, d, _lib.KNN_METRICS[metric], _tptr(ws), int(ws.numel()),
                                                  _tptr(order)))

    # -- GF-ICF
    def csc_count(self, G, n_cells, colptr, rowidx, x, nt):
        check(self.L.gficf_csc_count_device(self._bind(), G, n_cells, _tptr(colptr), _tptr(rowidx), _tptr(x),
                                            int(rowidx.numel()), _tptr(nt)))

    def csc_genes(self, G, N_total, nt, prop_min, prop_max, w_in, keep, genes, w, gkept):
        """genes: float64 tensor of genes_words(G) elements, raw storage for the per-gene tables."""
        check(self.L.gficf_csc_genes_device(self._bind(), G, N_total, _tptr(nt), float(prop_min), float(prop_max),
                                            _tptr(w_in), _tptr(keep), _tptr(genes), _tptr(w), _tptr(gkept)))

    def csc_colptr(self, G, n_cells, colptr, rowidx, keep, gkept, out_colptr):
        check(self.L.gficf_csc_colptr_device(self._bind(), G, n_cells, _tptr(colptr), _tptr(rowidx), _tptr(keep),
                                             _tptr(gkept), _tptr(out_colptr)))

    def csc_scale(self, G, n_cells, colptr, rowidx, x, genes, gkept, out_colptr, out_rowidx, out_x):
        check(self.L.gficf_csc_scale_device(self._bind(), G, n_cells, _tptr(colptr), _tptr(rowidx), _tptr(x),
                                            int(rowidx.numel()), _tptr(genes), _tptr(gkept), _tptr(out_colptr),
                                            _tptr(out_rowidx), _tptr(out_x)))

    # -- the chain in the pointerB / pointerE form (cells compact inside their own input range; no global positions, no kept-count pass)
    def csc_scale_be(self, G, n_cells, colptr, rowidx, x, genes, gkept, out_end, out_rowidx, out_x):
        check(self.L.gficf_csc_scale_be_device(self._bind(), G, n_cells, _tptr(colptr), _tptr(rowidx), _tptr(x), int(rowidx.numel()),
                                               _tptr(genes), _tptr(gkept), _tptr(out_end), _tptr(out_rowidx), _tptr(out_x)))

    def gficf_csc_be(self, G, N, colptr, rowidx, x, prop_min=0.05, prop_max=1.0, w_in=None, ws=None, exact: bool = False) -> dict:
        """:meth:`gficf_csc` with the matrix returned in the pointerB / pointerE form: cell c's kept entries are
        ``out_rowidx / out_x [colptr[c] : out_end[c]]`` (``ws["out_end"]``, int64[N]) — same entries, order and values as the
        canonical form, three launches instead of five.  :meth:`csc_transpose_be` and :meth:`cluster_signatures_be` read it."""
        ws = ws or self.csc_workspace(G, N, int(rowidx.numel()))
        if "out_end" not in ws:
            ws["out_end"] = self.torch.zeros(max(N, 1), dtype=self.torch.int64, device=f"cuda:{self.device}")
        check(self.L.gficf_csc_be_device(self._bind(), 1 if exact else 0, G, N, _tptr(colptr), _tptr(rowidx), _tptr(x), int(rowidx.numel()),
                                         float(prop_min), float(prop_max), _tptr(w_in), _tptr(ws["nt"]), _tptr(ws["keep"]), _tptr(ws["genes"]),
                                         _tptr(ws["w"]), _tptr(ws["gkept"]), _tptr(ws["out_end"]), _tptr(ws["out_rowidx"]), _tptr(ws["out_x"])))
        return ws

    def gficf_csc_prepared(self, G, N, colptr, rowidx, x, prop_min=0.05, prop_max=1.0, w_in=None, ws=None, form: str = "canonical"):
        """:meth:`gficf_csc` (``form="canonical"``) or :meth:`gficf_csc_be` (``form="begin_end"``) with every argument converted ONCE:
        returns ``(run, ws)``, ``run()`` being one call into the library per pass (the fast count: stored entries, ``x`` not read),
        on torch's current stream at the time of the call.  For passes of tens of microseconds (BASELINE configs 1 - 2), where
        building eighteen ctypes arguments costs as much as the five kernels."""
        ws = ws or self.csc_workspace(G, N, int(rowidx.numel()))
        ctx, cur = self.ctx, self.current_stream
        head = (_tptr(colptr), _tptr(rowidx), _tptr(x), int(rowidx.numel()), float(prop_min), float(prop_max), _tptr(w_in), _tptr(ws["nt"]),
                _tptr(ws["keep"]), _tptr(ws["genes"]), _tptr(ws["w"]), _tptr(ws["gkept"]))
        if form == "begin_end":
            if "out_end" not in ws:
                ws["out_end"] = self.torch.zeros(max(N, 1), dtype=self.torch.int64, device=f"cuda:{self.device}")
            fn = self.L.gficf_csc_be_device
            args = (ctx.handle, 0, int(G), int(N)) + head + (_tptr(ws["out_end"]), _tptr(ws["out_rowidx"]), _tptr(ws["out_x"]))
        elif form == "canonical":
            fn = self.L.gficf_csc_device
            args = (ctx.handle, int(G), int(N)) + head + (_tptr(ws["out_colptr"]), _tptr(ws["out_rowidx"]), _tptr(ws["out_x"]))
        else:
            raise ValueError("form must be 'canonical' or 'begin_end'")

        def run():
            s_ = cur()
            if s_ != ctx._stream:
                ctx.set_stream(s_)
            rc = fn(*args)
            if rc:
                check(rc)

        run.keep = (colptr, rowidx, x, w_in, ws)
        return run, ws

    def cluster_signatures_be(self, G, n_cells, col_begin, col_end, rowidx, x, cluster, C, out):
        check(self.L.gficf_cluster_signatures_be_device(self._bind(), G, n_cells, _tptr(col_begin), _tptr(col_end), _tptr(rowidx), _tptr(x),
                                                        _tptr(cluster), int(C), _tptr(out)))

    def csc_transpose_be(self, G, n_cells, col_begin, col_end, rowidx, x, out_ptr, out_idx, out_x, ws):
        """t() of a matrix in the pointerB / pointerE form; the result is a compact CSC (out_ptr[G] entries)."""
        check(self.L.gficf_csc_transpose_be_device(self._bind(), G, n_cells, _tptr(col_begin), _tptr(col_end), _tptr(rowidx), _tptr(x),
                                                   int(rowidx.numel()), _tptr(out_ptr), _tptr(out_idx), _tptr(out_x), _tptr(ws),
                                                   int(ws.numel() * ws.element_size())))

    def cluster_signatures(self, G, n_cells, colptr, rowidx, x, cluster, C, out):
        """out: (C, G) float64 == column-major G x C; cluster: int32 ids in [0, C)."""
        check(self.L.gficf_cluster_signatures_device(self._bind(), G, n_cells, _tptr(colptr), _tptr(rowidx), _tptr(x),
                                                     _tptr(cluster), int(C), _tptr(out)))

    @staticmethod
    def cluster_markers_workspace_bytes(G: int, N: int, nnz: int, C: int) -> int:
        """Device scratch of ``cluster_markers`` (libgficf_markers.so)."""
        from . import _markers_lib

        return int(_markers_lib.load().gficf_cluster_markers_workspace_bytes(int(G), int(N), int(nnz), int(C)))

    def cluster_markers(self, G, n_cells, colptr, rowidx, x, cluster, C, ws, p, lfc):
        """Marker-gene test on device-resident tensors (colptr int64, rowidx int32, x float64, cluster int32 ids in [0, C),
        ws uint8 of ``cluster_markers_workspace_bytes``); p, lfc: (C, G) float64 == column-major G x C.  Enqueues only: call
        ``cluster_markers_sync(ws)`` to wait and to collect the deferred input errors."""
        from . import _markers_lib

        check(_markers_lib.load().gficf_cluster_markers_device(self._bind(), int(G), int(n_cells), _tptr(colptr), _tptr(rowidx), _tptr(x),
                                                               int(rowidx.numel()), _tptr(cluster), int(C), _tptr(ws),
                                                               int(ws.numel() * ws.element_size()), _tptr(p), _tptr(lfc)))

    def cluster_markers_sync(self, ws):
        from . import _markers_lib

        check(_markers_lib.load().gficf_cluster_markers_sync(self._bind(), _tptr(ws)))

    @staticmethod
    def gsea_workspace_bytes(G: int, C: int, P: int, n_members: int, D: int, nsim: int) -> int:
        """Device scratch of ``gsea`` (libgficf_gsea.so)."""
        from . import _gsea_lib

        return int(_gsea_lib.load().gficf_gsea_workspace_bytes(int(G), int(C), int(P), int(n_members), int(D), int(nsim)))

    def gsea(self, G, C, stats, ptr, members, sizes, size_idx, nsim, seed, ws, es, nes, pval, null=None):
        """Gene-set enrichment on device-resident tensors (stats: (C, G) float64 == column-major G x C; ptr int64 of P + 1,
        members int32; sizes int32: the D distinct tested sizes, ascending; size_idx int32 per pathway, -1 = not tested; ws uint8
        of ``gsea_workspace_bytes``); es, nes, pval: (C, P) float64 == column-major P x C; null: (D, nsim) or None.  Enqueues
        only: call ``gsea_sync(ws)`` to wait and to collect the deferred input errors."""
        from . import _gsea_lib

        check(_gsea_lib.load().gficf_gsea_device(self._bind(), int(G), int(C), _tptr(stats), int(ptr.numel()) - 1, _tptr(ptr), _tptr(members),
                                                 int(members.numel()), int(sizes.numel()), _tptr(sizes), _tptr(size_idx), int(nsim),
                                                 int(seed) & 0xFFFFFFFF, _tptr(ws), int(ws.numel() * ws.element_size()), _tptr(es), _tptr(nes),
                                                 _tptr(pval), _tptr(null)))

    def gsea_sync(self, ws):
        from . import _gsea_lib

        check(_gsea_lib.load().gficf_gsea_sync(self._bind(), _tptr(ws)))

    @staticmethod
    def gsva_workspace_bytes(G: int, N: int, C: int, P: int) -> int:
        """Device scratch of ``gsva_density`` and ``gsva_scores`` (libgficf_gsva.so)."""
        from . import _gsva_lib

        return int(_gsva_lib.load().gficf_gsva_workspace_bytes(int(G), int(N), int(C), int(P)))

    def gsva_density(self, G, N, C, cluster, seg_ptr, cell, x, max_seg, ws, sd, d0, kept, dnz):
        """Stages 1-2 of GSVA on device-resident tensors (cluster int32 of N; seg_ptr int64 of G * C + 1, cell int32 and x float64:
        the entries grouped by (gene, cluster); ws uint8 of ``gsva_workspace_bytes``); sd, d0: (C, G) float64, kept: (C, G) int32,
        dnz: one float64 per entry.  Enqueues only: ``gsva_sync(ws)`` waits and collects the deferred input errors."""
        from . import _gsva_lib

        check(_gsva_lib.load().gficf_gsva_density_device(self._bind(), int(G), int(N), int(C), _tptr(cluster), _tptr(seg_ptr), _tptr(cell), _tptr(x),
                                                         int(x.numel()), int(max_seg), _tptr(ws), int(ws.numel() * ws.element_size()), _tptr(sd),
                                                         _tptr(d0), _tptr(kept), _tptr(dnz)))

    def gsva_scores(self, G, N, C, cluster, colptr, row, src, max_cell_nz, dnz, d0, kept, ptr, members, min_size, max_size, fresh, ws, es, tested,
                    ssum, ssq):
        """Stages 3-5 of GSVA and the per-cluster sums on device-resident tensors (colptr int64 of N + 1, row int32, src int64: the
        entries cell-major); es: (N, P) float64 == column-major P x N; tested int32, ssum, ssq float64: (C, P).  Enqueues only."""
        from . import _gsva_lib

        check(_gsva_lib.load().gficf_gsva_scores_device(self._bind(), int(G), int(N), int(C), _tptr(cluster), _tptr(colptr), _tptr(row), _tptr(src),
                                                        int(row.numel()), int(max_cell_nz), _tptr(dnz), _tptr(d0), _tptr(kept), int(ptr.numel()) - 1,
                                                        _tptr(ptr), _tptr(members), int(members.numel()), int(min_size), int(max_size), int(fresh),
                                                        _tptr(ws), int(ws.numel() * ws.element_size()), _tptr(es), _tptr(tested), _tptr(ssum), _tptr(ssq)))

    def gsva_sync(self, ws):
        from . import _gsva_lib

        check(_gsva_lib.load().gficf_gsva_sync(self._bind(), _tptr(ws)))

    @staticmethod
    def tmm_workspace_bytes(G: int, N: int, big_cells: int = 0, big_entries: int = 0) -> int:
        """Device scratch of ``tmm_stats``, ``tmm_factors`` and ``tmm_cpm`` (libgficf_tmm.so).  ``big_cells``, ``big_entries``: the
        cells with more stored entries than the LDS capacity (``_tmm_lib.LDS_N``, or ``max_lds_n``) and their entries together."""
        from . import _tmm_lib

        return int(_tmm_lib.load().gficf_tmm_workspace_bytes(int(G), int(N), int(big_cells), int(big_entries)))

    def tmm_stats(self, G, N, colptr, rowidx, x, max_cell_nz, ws, lib, sq, f75, ostat, gprime, max_lds_n: int = 0):
        """Stage 1 of TMM on device-resident tensors (colptr int32 or int64 of N + 1, rowidx int32, x float64; ws uint8 of
        ``tmm_workspace_bytes``): lib, sq, f75 float64 of N, ostat float64 (2, N), gprime int32 of 1.  Enqueues only:
        ``tmm_sync(ws)`` waits and collects the deferred input errors."""
        from . import _tmm_lib

        check(_tmm_lib.load().gficf_tmm_stats_device(self._bind(), int(G), int(N), _tptr(colptr), 1 if colptr.element_size() == 8 else 0, _tptr(rowidx),
                                                     _tptr(x), int(x.numel()), int(max_cell_nz), int(max_lds_n), _tptr(ws),
                                                     int(ws.numel() * ws.element_size()), _tptr(lib), _tptr(sq), _tptr(f75), _tptr(ostat), _tptr(gprime)))

    def tmm_factors(self, G, N, colptr, rowidx, x, max_cell_nz, ref_col, lib, ws, factor, n, kept, logratioTrim=.3, sumTrim=.05, doWeighting=True,
                    max_lds_n: int = 0, big_cells: int = 0, big_entries: int = 0, fresh: bool = True):
        """Stage 2 of TMM on device-resident tensors: the factor (float64, not yet normalised), n and kept (int32) of every
        cell against column ``ref_col``, from the library sizes ``lib``.  Enqueues only."""
        from . import _tmm_lib

        check(_tmm_lib.load().gficf_tmm_factors_device(self._bind(), int(G), int(N), _tptr(colptr), 1 if colptr.element_size() == 8 else 0, _tptr(rowidx),
                                                       _tptr(x), int(x.numel()), int(max_cell_nz), int(ref_col), _tptr(lib), float(logratioTrim),
                                                       float(sumTrim), 1 if doWeighting else 0, int(max_lds_n), int(big_cells), int(big_entries),
                                                       1 if fresh else 0, _tptr(ws), int(ws.numel() * ws.element_size()), _tptr(factor), _tptr(n),
                                                       _tptr(kept)))

    def tmm_cpm(self, N, colptr, x, lib, factor, ws, out):
        """Stage 3: ``out = x / (1e-6 * (lib * factor))`` per stored entry, on device-resident tensors.  Enqueues only."""
        from . import _tmm_lib

        check(_tmm_lib.load().gficf_tmm_cpm_device(self._bind(), int(N), _tptr(colptr), 1 if colptr.element_size() == 8 else 0, _tptr(x), int(x.numel()),
                                                   _tptr(lib), _tptr(factor), _tptr(ws), int(ws.numel() * ws.element_size()), _tptr(out)))

    def tmm_sync(self, ws):
        from . import _tmm_lib

        check(_tmm_lib.load().gficf_tmm_sync(self._bind(), _tptr(ws)))

    # -- exact tail of the enrichment score (libgficf_gsea_exact.so)
    @staticmethod
    def gsea_tail_workspace_bytes(G: int, n: int) -> int:
        """Device scratch of ``gsea_tail`` for ``n`` pairs among ``G`` genes."""
        from . import _gsea_exact_lib

        return int(_gsea_exact_lib.load().gficf_gsea_tail_workspace_bytes(int(G), int(n)))

    def gsea_tail(self, G, size, es, tail, ws):
        """The exact one-sided tails on device-resident tensors: size int32, es and tail float64 of n, ws uint8 of
        ``gsea_tail_workspace_bytes``.  Enqueues only: call ``gsea_tail_sync(ws)`` to wait and to collect the deferred input errors."""
        from . import _gsea_exact_lib

        if size.element_size() != 4 or es.element_size() != 8 or tail.element_size() != 8 or es.numel() != size.numel() or tail.numel() != size.numel():
            raise ValueError("size must be int32, es and tail float64, all of one length")
        check(_gsea_exact_lib.load().gficf_gsea_tail_device(self._bind(), int(G), int(size.numel()), _tptr(size), _tptr(es), _tptr(tail), _tptr(ws),
                                                            int(ws.numel() * ws.element_size())))

    def gsea_tail_sync(self, ws):
        from . import _gsea_exact_lib

        check(_gsea_exact_lib.load().gficf_gsea_tail_sync(self._bind(), _tptr(ws)))

    # -- highly variable genes (libgficf_hvg.so); every stage enqueues only: ``hvg_sync(ws)`` waits and collects the deferred errors
    @staticmethod
    def hvg_workspace_bytes(G: int, N: int = 0, nnz: int = 0, grid_pts: int = 0) -> int:
        """Device scratch of the ``hvg_*`` stages for lists of up to ``G`` values, the gene-major view of a G x N matrix of
        ``nnz`` entries (``hvg_moments`` only) and grids of up to ``grid_pts`` points (``hvg_curve_distance`` only)."""
        from . import _hvg_lib

        return int(_hvg_lib.load().gficf_hvg_workspace_bytes(int(G), int(N), int(nnz), int(grid_pts)))

    def hvg_moments(self, G, N, colptr, rowidx, x, ws, mean, sd, var, nobs, lx, ly, valid):
        """Step 1 on device-resident tensors (colptr int64 of N + 1, rowidx int32, x float64): mean, sd, var, lx, ly float64
        of G, nobs and valid int32 of G."""
        from . import _hvg_lib

        if colptr.element_size() != 8:
            raise ValueError("colptr must be int64")
        check(_hvg_lib.load().gficf_hvg_moments_device(self._bind(), int(G), int(N), _tptr(colptr), _tptr(rowidx), _tptr(x), int(x.numel()), _tptr(ws),
                                                       int(ws.numel() * ws.element_size()), _tptr(mean), _tptr(sd), _tptr(var), _tptr(nobs), _tptr(lx),
                                                       _tptr(ly), _tptr(valid)))

    def hvg_order(self, key, valid, ws, perm, count):
        """The stable ascending order of ``key`` (float64) into ``perm`` (int32), the positions with ``valid == 0`` last
        (``valid`` None: all count); ``count`` (int32 of 1): how many count."""
        from . import _hvg_lib

        check(_hvg_lib.load().gficf_hvg_order_device(self._bind(), int(key.numel()), _tptr(key), _tptr(valid), _tptr(ws),
                                                     int(ws.numel() * ws.element_size()), _tptr(perm), _tptr(count)))

    def hvg_locfit(self, xs, ys, w, k, at, ws, fit, h=None):
        """The local quadratic fit at the points ``at`` from the ascending ``xs``, ``ys`` and weights ``w`` (None: ones) over the
        ``k`` nearest; ``fit`` and ``h`` (optional): float64 of ``len(at)``."""
        from . import _hvg_lib

        check(_hvg_lib.load().gficf_hvg_locfit_device(self._bind(), int(xs.numel()), _tptr(xs), _tptr(ys), _tptr(w), int(k), int(at.numel()), _tptr(at),
                                                      _tptr(ws), int(ws.numel() * ws.element_size()), _tptr(fit), _tptr(h)))

    def hvg_robust(self, xs, ys, k, iters, ws, w, fit, s, w_in=None):
        """Cleveland's loop: ``iters + 1`` fits at the data, the weights from 1 (or ``w_in``); ``w``, ``fit``: float64 of n, ``s``: of iters."""
        from . import _hvg_lib

        check(_hvg_lib.load().gficf_hvg_robust_device(self._bind(), int(xs.numel()), _tptr(xs), _tptr(ys), _tptr(w_in), int(k), int(iters), _tptr(ws),
                                                      int(ws.numel() * ws.element_size()), _tptr(w), _tptr(fit), _tptr(s)))

    def hvg_gap(self, xs, x0, step, half, ws, grid, gap):
        """``grid[i] = x0 + i * step`` and the points of the ascending ``xs`` in ``[grid[i] - half, grid[i] + half)`` (int32)."""
        from . import _hvg_lib

        check(_hvg_lib.load().gficf_hvg_gap_device(self._bind(), int(xs.numel()), _tptr(xs), float(x0), float(step), float(half), int(grid.numel()),
                                                   _tptr(ws), int(ws.numel() * ws.element_size()), _tptr(grid), _tptr(gap)))

    def hvg_curve_distance(self, lx, ly, b, a, x0, grid_len, ws, cvdist, index=None):
        """Step 5: the signed distance of every (lx, ly) to the curve (b, a) on the grid ``x0 + i * 0.001``, ``i < grid_len``."""
        from . import _hvg_lib

        check(_hvg_lib.load().gficf_hvg_curve_distance_device(self._bind(), int(lx.numel()), _tptr(lx), _tptr(ly), float(b), float(a), float(x0),
                                                              int(grid_len), _tptr(ws), int(ws.numel() * ws.element_size()), _tptr(cvdist), _tptr(index)))

    def hvg_kde(self, v, ws, stats, dens, argmax):
        """Step 6: ``stats`` float64 of 8 (bw, distMid, grid lo, grid hi, sd, the quartiles, mean), ``dens`` float64 of 512,
        ``argmax`` int32 of 1."""
        from . import _hvg_lib

        check(_hvg_lib.load().gficf_hvg_kde_device(self._bind(), int(v.numel()), _tptr(v), _tptr(ws), int(ws.numel() * ws.element_size()), _tptr(stats),
                                                   _tptr(dens), _tptr(argmax)))

    def hvg_sync(self, ws):
        from . import _hvg_lib

        check(_hvg_lib.load().gficf_hvg_sync(self._bind(), _tptr(ws)))

    # -- Harmony (libgficf_harmony.so, include/gficf_harmony.h); all tensors float64 but ``levels``, ``perm``, ``labels`` (int32):
    # Z, Zc, Zcorr (N, d); levels (V, N); Y (K, d); R (K, N); O, E (K, B); theta, lamb (B,); ``var_start`` is a host int32 array
    # of V + 1; ``ws``: uint8 of ``harmony_workspace_bytes``.  Every stage only enqueues; ``harmony`` waits once a round for the
    # objective; ``harmony_sync(ws)`` waits and collects the deferred errors.
    @staticmethod
    def harmony_workspace_bytes(N: int, d: int, K: int, V: int, B: int) -> int:
        from . import _harmony_lib

        return int(_harmony_lib.load().gficf_harmony_workspace_bytes(int(N), int(d), int(K), int(V), int(B)))

    @staticmethod
    def _harmony_dims(Z, Y, levels, var_start):
        vs = np.ascontiguousarray(var_start, dtype=np.int32)
        V = int(levels.shape[0])
        if vs.shape != (V + 1,):
            raise ValueError("var_start must hold one entry per variable and the total")
        return int(Z.shape[0]), int(Z.shape[1]), int(Y.shape[0]), V, int(vs[-1]), vs

    def harmony_normalise(self, Z, Zc, ws):
        """Stage 1: ``Zc[i] = Z[i] / |Z[i]|``; starts the status word and the counters of ``ws`` again."""
        from . import _harmony_lib

        check(_harmony_lib.load().gficf_harmony_normalise_device(self._bind(), int(Z.shape[0]), int(Z.shape[1]), _tptr(Z), _tptr(Zc), _tptr(ws),
                                                                 int(ws.numel())))

    def harmony_start(self, Zc, Y0, init_iter, Y, labels, ws):
        """Stage 2: ``init_iter`` hard Lloyd iterations under cosine from ``Y0``."""
        from . import _harmony_lib

        check(_harmony_lib.load().gficf_harmony_start_device(self._bind(), int(Zc.shape[0]), int(Zc.shape[1]), int(Y0.shape[0]), _tptr(Zc), _tptr(Y0),
                                                             int(init_iter), _tptr(Y), _tptr(labels), _tptr(ws), int(ws.numel())))

    def harmony_assign(self, Zc, levels, var_start, Y, sigma, R, O, E, ws):
        """Stage 3: the soft assignments of ``Y`` without penalty, ``O = R Phi^T`` and ``E``."""
        from . import _harmony_lib

        N, d, K, V, B, vs = self._harmony_dims(Zc, Y, levels, var_start)
        check(_harmony_lib.load().gficf_harmony_assign_device(self._bind(), N, d, K, V, B, _np_ptr(vs), _tptr(Zc), _tptr(levels), _tptr(Y), float(sigma),
                                                              _tptr(R), _tptr(O), _tptr(E), _tptr(ws), int(ws.numel())))

    def harmony_round(self, Zc, levels, var_start, theta, sigma, perm, n_blocks, R, O, E, Y, ws):
        """Stage 4: one clustering round over the blocks of ``perm`` (N int32); R, O, E and Y are updated in place."""
        from . import _harmony_lib

        N, d, K, V, B, vs = self._harmony_dims(Zc, Y, levels, var_start)
        if perm.numel() != N:
            raise ValueError("perm must hold N entries")
        check(_harmony_lib.load().gficf_harmony_round_device(self._bind(), N, d, K, V, B, _np_ptr(vs), _tptr(Zc), _tptr(levels), _tptr(theta), float(sigma),
                                                             _tptr(perm), int(n_blocks), _tptr(R), _tptr(O), _tptr(E), _tptr(Y), _tptr(ws),
                                                             int(ws.numel())))

    def harmony_objective(self, Zc, levels, var_start, Y, R, O, E, theta, sigma, obj, ws):
        """Stage 5: the objective into ``obj`` (float64 of 1, on the device)."""
        from . import _harmony_lib

        N, d, K, V, B, vs = self._harmony_dims(Zc, Y, levels, var_start)
        check(_harmony_lib.load().gficf_harmony_objective_device(self._bind(), N, d, K, V, B, _np_ptr(vs), _tptr(Zc), _tptr(levels), _tptr(Y), _tptr(R),
                                                                 _tptr(O), _tptr(E), _tptr(theta), float(sigma), _tptr(obj), _tptr(ws), int(ws.numel())))

    def harmony_correct(self, Z, levels, var_start, R, lamb, Zcorr, ws, W=None):
        """Stage 6: ``Zcorr`` from the original ``Z``; ``W`` (K, B + 1, d), if given, gets the ridge coefficients."""
        from . import _harmony_lib

        N, d, K, V, B, vs = self._harmony_dims(Z, R, levels, var_start)
        check(_harmony_lib.load().gficf_harmony_correct_device(self._bind(), N, d, K, V, B, _np_ptr(vs), _tptr(Z), _tptr(levels), _tptr(R), _tptr(lamb),
                                                               _tptr(Zcorr), _tptr(W), _tptr(ws), int(ws.numel())))

    def harmony(self, Z, levels, var_start, theta, lamb, sigma, Y0, perm, init_iter, max_iter_harmony, max_iter_kmeans, n_blocks, epsilon_cluster,
                epsilon_harmony, Zcorr, Zc, R, Y, O, E, ws) -> dict:
        """Stage 7, the chain; ``perm`` (rounds, N) int32.  Returns ``objective`` (every round's, the one after stage 3 first),
        ``iter_rounds``, ``iterations``, ``rounds`` and ``converged``."""
        from . import _harmony_lib

        N, d, K, V, B, vs = self._harmony_dims(Z, Y0, levels, var_start)
        rounds = int(perm.shape[0]) if perm.dim() == 2 else 0
        if rounds and int(perm.shape[1]) != N:
            raise ValueError("perm must be (rounds, N)")
        objective = np.full(rounds + 1, np.nan, dtype=np.float64)
        iter_rounds = np.zeros(max(int(max_iter_harmony), 1), dtype=np.int32)
        info = np.zeros(4, dtype=np.int64)
        check(_harmony_lib.load().gficf_harmony_device(self._bind(), N, d, K, V, B, _np_ptr(vs), _tptr(Z), _tptr(levels), _tptr(theta), _tptr(lamb),
                                                       float(sigma), _tptr(Y0), _tptr(perm), rounds, int(init_iter), int(max_iter_harmony),
                                                       int(max_iter_kmeans), int(n_blocks), float(epsilon_cluster), float(epsilon_harmony), _tptr(Zcorr),
                                                       _tptr(Zc), _tptr(R), _tptr(Y), _tptr(O), _tptr(E), _np_ptr(objective), _np_ptr(iter_rounds),
                                                       _np_ptr(info), _tptr(ws), int(ws.numel())))
        return {"objective": objective[:1 + int(info[1])], "iter_rounds": iter_rounds[:int(info[0])], "iterations": int(info[0]),
                "rounds": int(info[1]), "converged": bool(info[2])}

    def harmony_sync(self, ws) -> dict:
        """Waits; raises the deferred errors; returns ``zero_rows`` and ``flat_clusters`` of the last normalisation and correction."""
        from . import _harmony_lib

        info = np.zeros(2, dtype=np.int64)
        check(_harmony_lib.load().gficf_harmony_sync(self._bind(), _tptr(ws), _np_ptr(info)))
        return {"zero_rows": int(info[0]), "flat_clusters": int(info[1])}

    # -- NMF (libgficf_nmf.so, include/gficf_nmf.h); dense operands float64, ROW-major with the pitch ``_nmf_lib.ld(k)`` (W: (G, ld),
    # H as its transpose: (N, ld)), a Gram matrix (lp, lp) with ``_nmf_lib.lp(k)``; colptr int64, rowidx int32, x float64; ``ws``: uint8
    # of ``nmf_workspace_bytes`` (``_nmf_lib.NNLS_WS_BYTES`` for ``nnls``), its first word zero before the first stage
    # (``torch.zeros``).  Every stage only enqueues; ``nmf`` waits once an iteration; ``nmf_sync(ws)`` waits and collects the
    # deferred errors.
    @staticmethod
    def nmf_workspace_bytes(G: int, N: int, nnz: int, k: int) -> int:
        """Device scratch of the ``nmf_*`` stages on a G x N (or N x G) matrix; 0 on sizes every stage refuses."""
        from . import _nmf_lib

        return int(_nmf_lib.load().gficf_nmf_workspace_bytes(int(G), int(N), int(nnz), int(k)))

    @staticmethod
    def _nmf_dense(k, **tensors):
        """Every named tensor (None: not given) is (rows, ld(k)) float64: the stages index them by that pitch."""
        from . import _nmf_lib

        for name, (t, rows) in tensors.items():
            if t is not None and (t.dim() != 2 or tuple(t.shape) != (int(rows), _nmf_lib.ld(k)) or t.element_size() != 8):
                raise ValueError(f"{name} must be a ({int(rows)}, {_nmf_lib.ld(k)}) float64 tensor for k = {k}, not {tuple(t.shape)}")

    @staticmethod
    def _nmf_small(k, S=None, sweeps=None, rows=0, counts=None, d=None):
        from . import _nmf_lib

        if S is not None and (S.dim() != 2 or S.shape[0] < _nmf_lib.lp(k) or S.shape[1] != _nmf_lib.lp(k)):
            raise ValueError(f"S must be ({_nmf_lib.lp(k)}, {_nmf_lib.lp(k)}) for k = {k}")
        if sweeps is not None and (sweeps.numel() < rows or sweeps.element_size() != 4):
            raise ValueError(f"sweeps must hold {rows} int32")
        if counts is not None and (counts.numel() < 2 or counts.element_size() != 8):
            raise ValueError("counts must hold 2 int64")
        if d is not None and (d.numel() < k or d.element_size() != 8):
            raise ValueError(f"d must hold {k} float64")

    def nnls(self, k, S, B, H0, cd_tol, cd_maxit, H, sweeps, ws):
        """The solve for ``k`` coordinates: S (>= k rows, >= k columns; its row stride is the pitch), B, H0 (or None: from
        zero), H (M, ld(k)); sweeps int32 of M."""
        from . import _nmf_lib

        k, M = int(k), int(B.shape[0])
        if S.dim() != 2 or S.shape[0] < k or S.shape[1] < k or S.element_size() != 8:
            raise ValueError(f"S must be a float64 matrix of at least {k} x {k}")
        self._nmf_dense(k, B=(B, M), H0=(H0, M), H=(H, M))
        self._nmf_small(k, sweeps=sweeps, rows=M)
        check(_nmf_lib.load().gficf_nnls_device(self._bind(), M, k, _tptr(S), int(S.stride(0)), _tptr(B), _tptr(H0), float(cd_tol), int(cd_maxit),
                                                _tptr(H), _tptr(sweeps), _tptr(ws), int(ws.numel())))

    def nmf_half(self, n_in, n_out, colptr, rowidx, x, nnz, k, X, Y, d, warm, l1, ridge, cd_tol, cd_maxit, ws, S=None, B=None, sweeps=None,
                 counts=None):
        """One half-step on a CSC matrix of n_in rows and n_out columns: X (n_in, ld) -> Y (n_out, ld), d (k), both also read
        with ``warm``.  Optional outputs: S (lp, lp), B (n_out, ld), sweeps int32 of n_out, counts int64 of 2 (dead, capped)."""
        from . import _nmf_lib

        self._nmf_dense(k, X=(X, n_in), Y=(Y, n_out), B=(B, n_out))
        self._nmf_small(k, S=S, sweeps=sweeps, rows=int(n_out), counts=counts, d=d)
        check(_nmf_lib.load().gficf_nmf_half_device(self._bind(), int(n_in), int(n_out), _tptr(colptr), _tptr(rowidx), _tptr(x), int(nnz), int(k),
                                                    _tptr(X), _tptr(Y), _tptr(d), 1 if warm else 0, float(l1), float(ridge), float(cd_tol),
                                                    int(cd_maxit), _tptr(S), _tptr(B), _tptr(sweeps), _tptr(counts), _tptr(ws), int(ws.numel())))

    def nmf_loss(self, G, N, colptr, rowidx, x, nnz, k, W, d, H, loss, ws):
        """``loss`` (float64 of 4): the loss, ``||A||^2``, the cross term, the quadratic term."""
        from . import _nmf_lib

        self._nmf_dense(k, W=(W, G), H=(H, N))
        self._nmf_small(k, d=d)
        if loss.numel() < 4 or loss.element_size() != 8:
            raise ValueError("loss must hold 4 float64")
        check(_nmf_lib.load().gficf_nmf_loss_device(self._bind(), int(G), int(N), _tptr(colptr), _tptr(rowidx), _tptr(x), int(nnz), int(k), _tptr(W),
                                                    _tptr(d), _tptr(H), _tptr(loss), _tptr(ws), int(ws.numel())))

    def nmf(self, G, N, colptr, rowidx, x, nnz, k, W0, tol, maxit, L1_w, L1_h, ridge, cd_tol, cd_maxit, track_loss, W, d, H, ws) -> dict:
        """The chain; W0 and W (G, ld) may be the same tensor.  Returns ``delta`` and ``loss`` (per iteration; ``loss`` None unless
        tracked), ``iterations``, ``converged``, ``dead`` and ``capped_rows``."""
        from . import _nmf_lib

        maxit = int(maxit)
        self._nmf_dense(k, W0=(W0, G), W=(W, G), H=(H, N))
        self._nmf_small(k, d=d)
        delta, loss, info = np.full(max(maxit, 1), np.nan), np.full(max(maxit, 1), np.nan), np.zeros(4, dtype=np.int64)
        check(_nmf_lib.load().gficf_nmf_device(self._bind(), int(G), int(N), _tptr(colptr), _tptr(rowidx), _tptr(x), int(nnz), int(k), _tptr(W0),
                                               float(tol), maxit, float(L1_w), float(L1_h), float(ridge), float(cd_tol), int(cd_maxit),
                                               1 if track_loss else 0, _tptr(W), _tptr(d), _tptr(H), _np_ptr(delta), _np_ptr(loss), _np_ptr(info),
                                               _tptr(ws), int(ws.numel())))
        it = int(info[0])
        return {"delta": delta[:it], "loss": loss[:it] if track_loss else None, "iterations": it, "converged": bool(info[1]), "dead": int(info[2]),
                "capped_rows": int(info[3])}

    def nmf_project(self, G, n_new, colptr, rowidx, x, nnz, k, W, ridge, cd_tol, cd_maxit, H, ws, S=None, B=None, sweeps=None):
        """New cells against W (G, ld): H (n_new, ld); optional outputs as in ``nmf_half``."""
        from . import _nmf_lib

        self._nmf_dense(k, W=(W, G), H=(H, n_new), B=(B, n_new))
        self._nmf_small(k, S=S, sweeps=sweeps, rows=int(n_new))
        check(_nmf_lib.load().gficf_nmf_project_device(self._bind(), int(G), int(n_new), _tptr(colptr), _tptr(rowidx), _tptr(x), int(nnz), int(k),
                                                       _tptr(W), float(ridge), float(cd_tol), int(cd_maxit), _tptr(H), _tptr(S), _tptr(B),
                                                       _tptr(sweeps), _tptr(ws), int(ws.numel())))

    def nmf_sync(self, ws):
        from . import _nmf_lib

        check(_nmf_lib.load().gficf_nmf_sync(self._bind(), _tptr(ws)))

    # -- overdispersed genes (libgficf_od.so); ``ws``: uint8 of ``od_workspace_bytes``, its first word zero before the first stage
    # (``torch.zeros``); ``od_fit`` and ``od_bh_log`` wait once for their host stage, the others only enqueue; ``od_sync(ws)``
    # waits and collects the deferred errors.  od_fit -> od_scores -> od_bh_log -> od_select_scale -> rsvd never leave the device.
    @staticmethod
    def od_workspace_bytes(G: int, N: int = 0) -> int:
        """Device scratch of the ``od_*`` stages for lists of up to ``G`` values and, for ``od_select_scale``, ``N`` columns."""
        from . import _od_lib

        return int(_od_lib.load().gficf_od_workspace_bytes(int(G), int(N)))

    def od_fit(self, m, var, nobs, ws, v, valid, fit, res, gam_k: int = 5, min_gene_cells: int = 0, sp=None) -> dict:
        """Steps 1 - 3 up to ``res`` (m, var float64 and nobs int32 of G; v, fit, res float64 and valid int32 of G).  Returns
        the fit's scalars (``_od_lib.INFO``)."""
        from . import _od_lib

        info = np.full(len(_od_lib.INFO), np.nan, dtype=np.float64)
        check(_od_lib.load().gficf_od_fit_device(self._bind(), int(m.numel()), _tptr(m), _tptr(var), _tptr(nobs), int(gam_k), int(min_gene_cells),
                                                 -1.0 if sp is None else float(sp), _tptr(ws), int(ws.numel() * ws.element_size()), _tptr(v),
                                                 _tptr(valid), _tptr(fit), _tptr(res), _np_ptr(info)))
        return dict(zip(_od_lib.INFO, info))

    def od_logpf(self, res, a, ws, lp):
        """``lp = log I_z(a, a)`` at ``z = 1 / (1 + exp(res))``, elementwise (float64)."""
        from . import _od_lib

        check(_od_lib.load().gficf_od_logpf_device(self._bind(), int(res.numel()), _tptr(res), _tptr(a), _tptr(ws), int(ws.numel() * ws.element_size()),
                                                   _tptr(lp)))

    def od_logqchisq(self, lp, df, ws, x):
        """``x = qchisq(lp, df, lower.tail = FALSE, log.p = TRUE)``, elementwise (float64)."""
        from . import _od_lib

        check(_od_lib.load().gficf_od_logqchisq_device(self._bind(), int(lp.numel()), _tptr(lp), float(df), _tptr(ws),
                                                       int(ws.numel() * ws.element_size()), _tptr(x)))

    def od_scores(self, res, nobs, v, N, ws, lp, qv, gsf, min_adjusted_variance: float = 1e-3, max_adjusted_variance: float = 1e3):
        """Steps 3, 5, 6: ``lp``, ``qv``, ``gsf`` (float64 of G) from ``res``, ``nobs`` (int32), ``v`` and the number of cells."""
        from . import _od_lib

        check(_od_lib.load().gficf_od_scores_device(self._bind(), int(res.numel()), _tptr(res), _tptr(nobs), _tptr(v), int(N), float(min_adjusted_variance),
                                                    float(max_adjusted_variance), _tptr(ws), int(ws.numel() * ws.element_size()), _tptr(lp), _tptr(qv),
                                                    _tptr(gsf)))

    def od_bh_log(self, lp, ws, lpa):
        """Step 4: ``lpa = bh.adjust(lp, log = TRUE)`` (float64 of G)."""
        from . import _od_lib

        check(_od_lib.load().gficf_od_bh_log_device(self._bind(), int(lp.numel()), _tptr(lp), _tptr(ws), int(ws.numel() * ws.element_size()), _tptr(lpa)))

    def od_select_scale(self, G, n_cells, colptr, rowidx, x, mask, scale, ws, out_colptr, out_rowidx, out_x, nsel):
        """The rows with ``mask != 0`` (int32 of G; None: all, only ``out_x`` is written) of the G x n_cells CSC (colptr int64),
        renumbered and multiplied by ``scale`` (float64 of G; None: 1): ``out_colptr`` int64 of n_cells + 1, ``out_rowidx``
        int32 and ``out_x`` float64 with room for the input's entries, ``nsel`` int32 of 1."""
        from . import _od_lib

        if colptr.element_size() != 8:
            raise ValueError("colptr must be int64")
        check(_od_lib.load().gficf_od_select_scale_device(self._bind(), int(G), int(n_cells), _tptr(colptr), _tptr(rowidx), _tptr(x), int(x.numel()),
                                                          _tptr(mask), _tptr(scale), _tptr(ws), int(ws.numel() * ws.element_size()), _tptr(out_colptr),
                                                          _tptr(out_rowidx), _tptr(out_x), _tptr(nsel)))

    def od_sync(self, ws):
        from . import _od_lib

        check(_od_lib.load().gficf_od_sync(self._bind(), _tptr(ws)))

    @staticmethod
    def rsvd_workspace_bytes(G: int, N: int, nnz: int, l: int) -> int:
        """Device scratch of ``rsvd`` (libgficf_pca.so)."""
        from . import _pca_lib

        return int(_pca_lib.load().gficf_rsvd_workspace_bytes(int(G), int(N), int(nnz), int(l)))

    def rsvd(self, G, n_cells, colptr, rowidx, x, centre, omega, k, l, q, ws, d, cells, genes, mean=None):
        """Randomized SVD on device-resident tensors (colptr int64, rowidx int32, x float64: the genes x cells CSC matrix;
        omega: (l, min(N, G)) float64 == column-major min(N, G) x l; ws uint8 of ``rsvd_workspace_bytes``); d: k, cells: (k, N),
        genes: (k, G), mean: G (with ``centre``) float64.  Enqueues only: call ``rsvd_sync(ws)`` to wait and to collect the
        deferred input errors."""
        from . import _pca_lib

        check(_pca_lib.load().gficf_rsvd_device(self._bind(), int(G), int(n_cells), _tptr(colptr), _tptr(rowidx), _tptr(x), int(rowidx.numel()),
                                                1 if centre else 0, _tptr(omega), int(k), int(l), int(q), _tptr(ws),
                                                int(ws.numel() * ws.element_size()), _tptr(d), _tptr(cells), _tptr(genes), _tptr(mean)))

    def rsvd_sync(self, ws):
        from . import _pca_lib

        check(_pca_lib.load().gficf_rsvd_sync(self._bind(), _tptr(ws)))

    @staticmethod
    def svds_workspace_bytes(G: int, N: int, nnz: int, k: int, b: int, m: int) -> int:
        """Device scratch of ``svds`` (libgficf_svds.so); 0 on arguments it would refuse."""
        from . import _svds_lib

        return int(_svds_lib.load().gficf_svds_workspace_bytes(int(G), int(N), int(nnz), int(k), int(b), int(m)))

    def svds(self, G, n_cells, colptr, rowidx, x, centre, start, k, b, m, tol, max_cycles, ws, d, cells, genes, residuals, info, mean=None):
        """Exact truncated SVD on device-resident tensors (colptr int64, rowidx int32, x float64: the genes x cells CSC matrix;
        start: (b, min(N, G)) float64 == column-major min(N, G) x b; ws uint8 of ``svds_workspace_bytes``); d: k, cells: (k, N),
        genes: (k, G), residuals: k, mean: G (with ``centre``) float64, info: 4 int64 (cycles, products, n_converged,
        exhausted).  Reads 5 integers back per restart cycle and only enqueues otherwise: call ``svds_sync(ws)`` to wait and to
        collect the deferred input errors."""
        from . import _svds_lib

        check(_svds_lib.load().gficf_svds_device(self._bind(), int(G), int(n_cells), _tptr(colptr), _tptr(rowidx), _tptr(x), int(rowidx.numel()),
                                                 1 if centre else 0, _tptr(start), int(k), int(b), int(m), float(tol), int(max_cycles), _tptr(ws),
                                                 int(ws.numel() * ws.element_size()), _tptr(d), _tptr(cells), _tptr(genes), _tptr(mean),
                                                 _tptr(residuals), _tptr(info)))

    def svds_sync(self, ws):
        from . import _svds_lib

        check(_svds_lib.load().gficf_svds_sync(self._bind(), _tptr(ws)))

    @staticmethod
    def sparse_knn_workspace_bytes(G: int, N: int, nnz: int, k: int, n_queries: int) -> int:
        """Device scratch of ``sparse_knn`` (libgficf_sparse_knn.so); 0 on arguments it would refuse."""
        from . import _sparse_knn_lib

        return int(_sparse_knn_lib.load().gficf_sparse_knn_workspace_bytes(int(G), int(N), int(nnz), int(k), int(n_queries)))

    def sparse_knn(self, G, n_cells, colptr, rowidx, x, k, metric, q_begin, q_end, ws, idx_cm, dist_cm=None):
        """Exact kNN of the cells [q_begin, q_end) among all ``n_cells`` sparse cells on device-resident tensors (colptr int64,
        rowidx int32, x float64: the genes x cells CSC matrix; ws uint8 of ``sparse_knn_workspace_bytes``); idx_cm: (k, ld) int32,
        contiguous, ld >= n_q == column-major n_q x k with leading dimension ld (the entries [n_q, ld) of a row are not written),
        1-based; dist_cm alike, float64, optional.  Enqueues only: call ``sparse_knn_sync(ws)`` to wait and to collect the deferred
        input errors."""
        from . import _sparse_knn_lib

        n_q = int(q_end) - int(q_begin)
        if idx_cm.dim() != 2 or idx_cm.shape[0] != int(k) or idx_cm.shape[1] < max(n_q, 1) or not idx_cm.is_contiguous():
            raise ValueError("idx_cm must be a contiguous (k, ld) tensor with ld >= the number of queries")
        if dist_cm is not None and (dist_cm.shape != idx_cm.shape or not dist_cm.is_contiguous()):
            raise ValueError("dist_cm must be contiguous and shaped like idx_cm")
        check(_sparse_knn_lib.load().gficf_sparse_knn_device(self._bind(), int(G), int(n_cells), _tptr(colptr), _tptr(rowidx), _tptr(x),
                                                             int(rowidx.numel()), int(k), _lib.KNN_METRICS[metric], int(q_begin), int(q_end),
                                                             _tptr(ws), int(ws.numel() * ws.element_size()), _tptr(idx_cm), _tptr(dist_cm),
                                                             int(idx_cm.shape[1])))

    def sparse_knn_sync(self, ws):
        from . import _sparse_knn_lib

        check(_sparse_knn_lib.load().gficf_sparse_knn_sync(self._bind(), _tptr(ws)))

    @staticmethod
    def sparse_query_workspace_bytes(G: int, N: int, nnz_train: int, M: int, nnz_query: int, k: int) -> int:
        """Device scratch of ``sparse_query`` (libgficf_sparse_query.so); 0 on arguments it would refuse."""
        from . import _sparse_query_lib

        return int(_sparse_query_lib.load().gficf_sparse_query_workspace_bytes(int(G), int(N), int(nnz_train), int(M), int(nnz_query), int(k)))

    def sparse_query(self, G, n_train, t_colptr, t_rowidx, t_x, n_query, q_colptr, q_rowidx, q_x, k, metric, ws, idx_cm, dist_cm=None,
                     dist32_cm=None):
        """Exact kNN of the ``n_query`` sparse cells of one genes x cells CSC matrix among the ``n_train`` of another, both
        device-resident (colptr int64, rowidx int32, x float64; ws uint8 of ``sparse_query_workspace_bytes``); idx_cm: (k, ld)
        int32, contiguous, ld >= n_query == column-major n_query x k with leading dimension ld (the entries [n_query, ld) of a row
        are not written), 1-based training ids; dist_cm (float64) and dist32_cm (float32) alike, each optional.  Enqueues only:
        call ``sparse_query_sync(ws)`` to wait and to collect the deferred input errors of both matrices."""
        from . import _sparse_query_lib

        n_query = int(n_query)
        if idx_cm.dim() != 2 or idx_cm.shape[0] != int(k) or idx_cm.shape[1] < max(n_query, 1) or not idx_cm.is_contiguous():
            raise ValueError("idx_cm must be a contiguous (k, ld) tensor with ld >= the number of queries")
        for name, t, dt in (("dist_cm", dist_cm, self.torch.float64), ("dist32_cm", dist32_cm, self.torch.float32)):
            if t is not None and (t.shape != idx_cm.shape or not t.is_contiguous() or t.dtype != dt):
                raise ValueError(f"{name} must be contiguous, {dt} and shaped like idx_cm")
        check(_sparse_query_lib.load().gficf_sparse_query_device(
            self._bind(), int(G), int(n_train), _tptr(t_colptr), _tptr(t_rowidx), _tptr(t_x), int(t_rowidx.numel()), n_query, _tptr(q_colptr),
            _tptr(q_rowidx), _tptr(q_x), int(q_rowidx.numel()), int(k), _lib.KNN_METRICS[metric], _tptr(ws), int(ws.numel() * ws.element_size()),
            _tptr(idx_cm), _tptr(dist_cm), _tptr(dist32_cm), int(idx_cm.shape[1])))

    def sparse_query_sync(self, ws):
        from . import _sparse_query_lib

        check(_sparse_query_lib.load().gficf_sparse_query_sync(self._bind(), _tptr(ws)))

    @staticmethod
    def csc_tmm_workspace_bytes(nrows: int, ncols: int, nnz: int, l: int) -> int:
        from . import _pca_lib

        return int(_pca_lib.load().gficf_csc_tmm_workspace_bytes(int(nrows), int(ncols), int(nnz), int(l)))

    def csc_tmm(self, nrows, ncols, colptr, rowidx, x, X, l, ws, Y):
        """``Y = t(A) X`` for the nrows x ncols CSC matrix A; X: (l, nrows), Y: (l, ncols) float64 == column-major nrows x l and
        ncols x l.  Enqueues only (``rsvd_sync(ws)`` collects the deferred errors)."""
        from . import _pca_lib

        check(_pca_lib.load().gficf_csc_tmm_device(self._bind(), int(nrows), int(ncols), _tptr(colptr), _tptr(rowidx), _tptr(x),
                                                   int(rowidx.numel()), _tptr(X), int(l), _tptr(ws), int(ws.numel() * ws.element_size()), _tptr(Y)))

    @staticmethod
    def orthonormalize_workspace_bytes(m: int, l: int) -> int:
        from . import _pca_lib

        return int(_pca_lib.load().gficf_orthonormalize_workspace_bytes(int(m), int(l)))

    def orthonormalize(self, m, l, Y, ws):
        """``orth`` in place on Y: (l, m) float64 == column-major m x l (include/gficf_pca.h).  Enqueues only."""
        from . import _pca_lib

        check(_pca_lib.load().gficf_orthonormalize_device(self._bind(), int(m), int(l), _tptr(Y), _tptr(ws), int(ws.numel() * ws.element_size())))

    @staticmethod
    def umap_graph_workspace_bytes(N: int, k: int) -> int:
        """Device scratch of ``umap_graph`` (libgficf_umap.so)."""
        from . import _umap_lib

        return int(_umap_lib.load().gficf_umap_graph_workspace_bytes(int(N), int(k)))

    def umap_graph(self, idx_cm, dist_cm, N, k, ws, rowptr, col, val, nnz, set_op_mix_ratio=1.0, local_connectivity=1.0, sigma=None, rho=None, w=None):
        """UMAP's fuzzy graph from the search's own output (idx_cm int32 / dist_cm float32: (k, ld) == column-major N x k, as
        ``knn_search`` writes them): rowptr int64 N + 1, col int32 / val float32 of at least 2 N k entries, nnz int64 (1), sigma /
        rho float32 N or None, w (the memberships, (k, N) float32 == column-major N x k) or None.  Enqueues only: ``umap_sync(ws)`` waits and collects the deferred input errors."""
        from . import _umap_lib

        ld = idx_cm.shape[1] if idx_cm.dim() == 2 else N
        check(_umap_lib.load().gficf_umap_graph_device(self._bind(), _tptr(idx_cm), _tptr(dist_cm), int(N), int(k), int(ld),
                                                       float(local_connectivity), float(set_op_mix_ratio), _tptr(ws),
                                                       int(ws.numel() * ws.element_size()), _tptr(rowptr), _tptr(col), _tptr(val),
                                                       int(min(col.numel(), val.numel())), _tptr(nnz), _tptr(sigma), _tptr(rho), _tptr(w)))

    @staticmethod
    def umap_layout_workspace_bytes(N: int, capacity: int) -> int:
        from . import _umap_lib

        return int(_umap_lib.load().gficf_umap_layout_workspace_bytes(int(N), int(capacity)))

    def umap_layout(self, N, rowptr, col, val, capacity, a, b, gamma, learning_rate, negative_sample_rate, n_epochs, epoch_begin, epoch_end, seed,
                    Y, ws):
        """Epochs [epoch_begin, epoch_end) of n_epochs of the layout, in place on Y ((N, 2) float32), over the graph of
        ``umap_graph`` (``capacity``: the entries of col / val that may be read).  One launch per epoch; enqueues only."""
        from . import _umap_lib

        check(_umap_lib.load().gficf_umap_layout_device(self._bind(), int(N), _tptr(rowptr), _tptr(col), _tptr(val), int(capacity), float(a),
                                                        float(b), float(gamma), float(learning_rate), int(negative_sample_rate), int(n_epochs),
                                                        int(epoch_begin), int(epoch_end), int(seed) & 0xFFFFFFFFFFFFFFFF, _tptr(Y), _tptr(ws),
                                                        int(ws.numel() * ws.element_size())))

    def umap_sync(self, ws):
        from . import _umap_lib

        check(_umap_lib.load().gficf_umap_sync(self._bind(), _tptr(ws)))

    # -- spectral start (libgficf_spectral.so)
    @staticmethod
    def graph_components_workspace_bytes(N: int) -> int:
        """Device scratch of ``graph_components`` (libgficf_spectral.so)."""
        from . import _spectral_lib

        return int(_spectral_lib.load().gficf_graph_components_workspace_bytes(int(N)))

    def graph_components(self, N, rowptr, col, capacity, labels, info, ws):
        """The connected components of a CSR graph (rowptr int64 N + 1, col int32, ``capacity`` entries that may be read): labels int32
        N (the smallest vertex id of each vertex's component), info int64 (2) = {components, rounds}.  Synchronises once per round; a
        bad row pointer or column is raised here."""
        from . import _spectral_lib

        check(_spectral_lib.load().gficf_graph_components_device(self._bind(), int(N), _tptr(rowptr), _tptr(col), int(capacity), _tptr(labels),
                                                                 _tptr(info), _tptr(ws), int(ws.numel() * ws.element_size())))

    @staticmethod
    def spectral_workspace_bytes(N: int, capacity: int, ndim: int, m: int = 32) -> int:
        from . import _spectral_lib

        return int(_spectral_lib.load().gficf_spectral_workspace_bytes(int(N), int(capacity), int(ndim), int(m)))

    def spectral(self, N, rowptr, col, val, capacity, ndim, start, tol, m, max_restarts, ws, theta, resid, vectors, info):
        """The ndim leading eigenpairs of S = D^-1/2 P D^-1/2 beside its trivial one (include/gficf_spectral.h): start and vectors (N,
        ndim) float64, theta / resid float64 (ndim), info int64 (4) = {components, restarts, multiplications, converged}.  With more
        than one component theta, resid and vectors are left untouched.  Synchronises once per restart cycle."""
        from . import _spectral_lib

        check(_spectral_lib.load().gficf_spectral_device(self._bind(), int(N), _tptr(rowptr), _tptr(col), _tptr(val), int(capacity), int(ndim),
                                                         _tptr(start), float(tol), int(m), int(max_restarts), _tptr(ws),
                                                         int(ws.numel() * ws.element_size()), _tptr(theta), _tptr(resid), _tptr(vectors),
                                                         _tptr(info)))

    # -- t-SNE (libgficf_tsne.so)
    @staticmethod
    def tsne_affinities_workspace_bytes(N: int, k: int) -> int:
        """Device scratch of ``tsne_affinities`` (libgficf_tsne.so)."""
        from . import _tsne_lib

        return int(_tsne_lib.load().gficf_tsne_affinities_workspace_bytes(int(N), int(k)))

    def tsne_affinities(self, idx_cm, dist_cm, N, k, perplexity, ws, rowptr, col, val, nnz, beta=None, pc=None):
        """t-SNE's P from the search's own output (idx_cm int32 / dist_cm float32: (k, ld) == column-major N x k, k = floor(3
        perplexity) + 1, euclidean): rowptr int64 N + 1, col int32 / val float32 of at least 2 N (k - 1) entries, nnz int64 (1),
        beta float64 N or None, pc (the conditionals, (k - 1, N) float32) or None.  Enqueues only: ``tsne_sync(ws)`` waits and
        collects the deferred input errors."""
        from . import _tsne_lib

        ld = idx_cm.shape[1] if idx_cm.dim() == 2 else N
        check(_tsne_lib.load().gficf_tsne_affinities_device(self._bind(), _tptr(idx_cm), _tptr(dist_cm), int(N), int(k), int(ld), float(perplexity),
                                                            _tptr(ws), int(ws.numel() * ws.element_size()), _tptr(rowptr), _tptr(col), _tptr(val),
                                                            int(min(col.numel(), val.numel())), _tptr(nnz), _tptr(beta), _tptr(pc)))

    @staticmethod
    def tsne_layout_workspace_bytes(N: int, capacity: int) -> int:
        """Device scratch of ``tsne_gradient`` and ``tsne_layout``."""
        from . import _tsne_lib

        return int(_tsne_lib.load().gficf_tsne_layout_workspace_bytes(int(N), int(capacity)))

    def tsne_gradient(self, N, rowptr, col, val, capacity, Y, exaggeration, ws, dC, rep=None, Z=None, kl=None):
        """dC ((N, 2) float32) = exaggeration x attr - rep / Z at Y ((N, 2) float32) over P; rep (N, 2) float32 or None, Z float64
        (1), kl float64 (1) or None.  Enqueues only."""
        from . import _tsne_lib

        check(_tsne_lib.load().gficf_tsne_gradient_device(self._bind(), int(N), _tptr(rowptr), _tptr(col), _tptr(val), int(capacity), _tptr(Y),
                                                          float(exaggeration), _tptr(ws), int(ws.numel() * ws.element_size()), _tptr(dC),
                                                          _tptr(rep), _tptr(Z), _tptr(kl)))

    def tsne_layout(self, N, rowptr, col, val, capacity, max_iter, iter_begin, iter_end, stop_lying_iter, mom_switch_iter, momentum,
                    final_momentum, eta, exaggeration_factor, Y, uY, gains, ws, kl=None):
        """Iterations [iter_begin, iter_end) of max_iter in place on Y, uY and gains ((N, 2) float32 each); kl float64 (1) or None.
        Three launches per iteration; enqueues only."""
        from . import _tsne_lib

        check(_tsne_lib.load().gficf_tsne_layout_device(self._bind(), int(N), _tptr(rowptr), _tptr(col), _tptr(val), int(capacity), int(max_iter),
                                                        int(iter_begin), int(iter_end), int(stop_lying_iter), int(mom_switch_iter),
                                                        float(momentum), float(final_momentum), float(eta), float(exaggeration_factor), _tptr(Y),
                                                        _tptr(uY), _tptr(gains), _tptr(ws), int(ws.numel() * ws.element_size()), _tptr(kl)))

    def tsne_sync(self, ws):
        from . import _tsne_lib

        check(_tsne_lib.load().gficf_tsne_sync(self._bind(), _tptr(ws)))

    # -- new cells (libgficf_transform.so); every *_workspace_bytes scratch begins with the status word transform_sync reads
    @staticmethod
    def transform_workspace_bytes(stage: str, M: int, N: int = 0, k: int = 1) -> int:
        """Device scratch of ``transform_<stage>``: stage is search (needs N), weights, init, layout or vote."""
        from . import _transform_lib

        L = _transform_lib.load()
        if stage == "search":
            return int(L.gficf_transform_search_workspace_bytes(int(M), int(N), int(k)))
        return int(getattr(L, f"gficf_transform_{stage}_workspace_bytes")(int(M), int(k)))

    def transform_search_split(self, M: int, N: int) -> int:
        """The slices the candidate range is cut into for M queries against N training rows."""
        from . import _transform_lib

        return int(_transform_lib.load().gficf_transform_search_split(self.ctx.handle, int(M), int(N)))

    def transform_search(self, train, N, query, M, d, k, metric, ws, idx_cm, dist_cm=None):
        """train (N, dpad) / query (M, dpad) float32 as ``knn_prepare`` writes them; idx_cm int32 / dist_cm float32 (or None):
        (k, ld) == column-major M x k, 1-based training ids.  Enqueues only, like every transform_* stage."""
        from . import _transform_lib

        ld = idx_cm.shape[1] if idx_cm.dim() == 2 else M
        check(_transform_lib.load().gficf_transform_search_device(self._bind(), _tptr(train), int(N), _tptr(query), int(M), int(d), int(k),
                                                                  _lib.KNN_METRICS[metric], _tptr(ws), int(ws.numel() * ws.element_size()),
                                                                  _tptr(idx_cm), _tptr(dist_cm), int(ld)))

    def transform_weights(self, idx_cm, dist_cm, N, M, k, ws, w_cm, local_connectivity=1.0, sigma=None, rho=None):
        """The memberships of the search's table: w_cm (k, ld_w) float32 == column-major M x k; sigma / rho float32 M or None."""
        from . import _transform_lib

        check(_transform_lib.load().gficf_transform_weights_device(self._bind(), _tptr(idx_cm), _tptr(dist_cm), int(N), int(M), int(k),
                                                                   int(idx_cm.shape[1]), float(local_connectivity), _tptr(ws),
                                                                   int(ws.numel() * ws.element_size()), _tptr(w_cm), int(w_cm.shape[1]),
                                                                   _tptr(sigma), _tptr(rho)))

    def transform_init(self, idx_cm, w_cm, Y_train, N, M, k, ws, Y):
        """Y ((M, 2) float32) = the membership-weighted mean of the k heads' positions in Y_train ((N, 2) float32)."""
        from . import _transform_lib

        check(_transform_lib.load().gficf_transform_init_device(self._bind(), _tptr(idx_cm), int(idx_cm.shape[1]), _tptr(w_cm), int(w_cm.shape[1]),
                                                                _tptr(Y_train), int(N), int(M), int(k), _tptr(ws),
                                                                int(ws.numel() * ws.element_size()), _tptr(Y)))

    def transform_layout(self, idx_cm, w_cm, Y_train, N, M, k, a, b, gamma, learning_rate, negative_sample_rate, n_epochs, epoch_begin, epoch_end,
                         seed, query_offset, Y, ws):
        """Epochs [epoch_begin, epoch_end) of n_epochs in place on Y ((M, 2) float32); Y_train is read only.  One launch."""
        from . import _transform_lib

        check(_transform_lib.load().gficf_transform_layout_device(self._bind(), _tptr(idx_cm), int(idx_cm.shape[1]), _tptr(w_cm),
                                                                  int(w_cm.shape[1]), _tptr(Y_train), int(N), int(M), int(k), float(a), float(b),
                                                                  float(gamma), float(learning_rate), int(negative_sample_rate), int(n_epochs),
                                                                  int(epoch_begin), int(epoch_end), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                                  int(query_offset), _tptr(Y), _tptr(ws), int(ws.numel() * ws.element_size())))

    def transform_vote(self, idx_cm, labels, N, M, k, C, ws, pred, votes=None):
        """pred (M int32) = the majority label among labels[idx - 1] (int32 N, in [0, C)); votes: (M, C) int32 or None."""
        from . import _transform_lib

        check(_transform_lib.load().gficf_transform_vote_device(self._bind(), _tptr(idx_cm), int(idx_cm.shape[1]), _tptr(labels), int(N), int(M),
                                                                int(k), int(C), _tptr(ws), int(ws.numel() * ws.element_size()), _tptr(pred),
                                                                _tptr(votes)))

    def transform_sync(self, ws):
        from . import _transform_lib

        check(_transform_lib.load().gficf_transform_sync(self._bind(), _tptr(ws)))

    def louvain_workspace_bytes(self, N: int, nnz: int, n_start: int = 1) -> int:
        """Device scratch of ``louvain``: with ``n_start`` given, enough for min(n_start, 16) starts to run together (one launch set)."""
        return int(self.L.gficf_louvain_workspace_bytes(int(N), int(nnz), int(n_start)))

    def louvain(self, N, indptr, indices, x, resolution, n_iter, labels, ws, algorithm: int = 1, n_start: int = 1, seed: int = 0):
        """Community detection on a device-resident symmetric adjacency matrix (indptr int64, indices int32, x float64).
        Returns (n_clusters, modularity); labels: int32[N]."""
        nc, q = ctypes.c_int64(0), ctypes.c_double(0.0)
        check(self.L.gficf_louvain_device(self._bind(), int(N), _tptr(indptr), _tptr(indices), _tptr(x), int(indices.numel()),
                                          float(resolution), int(algorithm), int(n_start), int(n_iter), int(seed), _tptr(labels), ctypes.byref(nc),
                                          ctypes.byref(q),
                                          _tptr(ws), int(ws.numel() * ws.element_size())))
        return nc.value, q.value

    def leiden_workspace_bytes(self, N: int, nnz: int) -> int:
        """Device scratch of ``leiden`` and ``leiden_refine``."""
        from . import _leiden_lib

        return int(_leiden_lib.load().gficf_leiden_workspace_bytes(int(N), int(nnz)))

    def leiden(self, N, indptr, indices, x, resolution, n_iterations, labels, ws, seed: int = 0, init=None):
        """Leiden on a device-resident symmetric adjacency matrix (indptr int64, indices int32, x float64); init: int32[N] or None.
        Returns (n_clusters, modularity); labels: int32[N]."""
        from . import _leiden_lib

        nc, q = ctypes.c_int64(0), ctypes.c_double(0.0)
        check(_leiden_lib.load().gficf_leiden_device(self._bind(), int(N), _tptr(indptr), _tptr(indices), _tptr(x), int(indices.numel()),
                                                     float(resolution), int(n_iterations), int(seed), _tptr(init), _tptr(labels), ctypes.byref(nc),
                                                     ctypes.byref(q), _tptr(ws), int(ws.numel() * ws.element_size())))
        return nc.value, q.value

    def leiden_refine(self, N, indptr, indices, x, resolution, labels_in, refined, ws):
        """The refinement stage alone; refined: int32[N], the smallest member id of every vertex's refined community.  Returns their number."""
        from . import _leiden_lib

        nr = ctypes.c_int64(0)
        check(_leiden_lib.load().gficf_leiden_refine_device(self._bind(), int(N), _tptr(indptr), _tptr(indices), _tptr(x), int(indices.numel()),
                                                            float(resolution), _tptr(labels_in), _tptr(refined), ctypes.byref(nr), _tptr(ws),
                                                            int(ws.numel() * ws.element_size())))
        return nr.value

    def slm_workspace_bytes(self, N: int, nnz: int) -> int:
        """Device scratch of ``slm`` and ``slm_submove``."""
        from . import _slm_lib

        return int(_slm_lib.load().gficf_slm_workspace_bytes(int(N), int(nnz)))

    def slm(self, N, indptr, indices, x, resolution, n_start, n_iter, labels, ws, seed: int = 0, init=None):
        """Smart local moving on a device-resident symmetric adjacency matrix (indptr int64, indices int32, x float64); init: int32[N]
        or None.  Returns (n_clusters, modularity, start, iterations); labels: int32[N]."""
        from . import _slm_lib

        info = _slm_lib.Info()
        check(_slm_lib.load().gficf_slm_device(self._bind(), int(N), _tptr(indptr), _tptr(indices), _tptr(x), int(indices.numel()), float(resolution),
                                               int(n_start), int(n_iter), int(seed) & 0xFFFFFFFF, _tptr(init), _tptr(ws),
                                               int(ws.numel() * ws.element_size()), _tptr(labels), ctypes.byref(info)))
        return info.n_clusters, info.modularity, info.start, info.iterations

    def slm_submove(self, N, indptr, indices, x, resolution, labels_in, sub, ws, seed: int = 0, level: int = 0):
        """The sub-moving stage alone; sub: int32[N], the smallest member id of every vertex's sub-community.  Returns (their number, passes)."""
        from . import _slm_lib

        info = _slm_lib.SubmoveInfo()
        check(_slm_lib.load().gficf_slm_submove_device(self._bind(), int(N), _tptr(indptr), _tptr(indices), _tptr(x), int(indices.numel()),
                                                       float(resolution), _tptr(labels_in), int(seed) & 0xFFFFFFFF, int(level), _tptr(ws),
                                                       int(ws.numel() * ws.element_size()), _tptr(sub), ctypes.byref(info)))
        return info.n_sub, info.passes

    def csc_transpose_workspace_bytes(self, G: int, n_cells: int) -> int:
        return int(self.L.gficf_csc_transpose_workspace_bytes(int(G), int(n_cells)))

    def csc_transpose(self, G, n_cells, colptr, rowidx, x, out_ptr, out_idx, out_x, ws):
        """t(gficf): out_ptr int64[G + 1], out_idx int32[nnz] (cells, ascending within a gene), out_x float64[nnz];
        ws: a uint8 tensor of csc_transpose_workspace_bytes(G, n_cells) bytes."""
        check(self.L.gficf_csc_transpose_device(self._bind(), G, n_cells, _tptr(colptr), _tptr(rowidx), _tptr(x),
                                                int(rowidx.numel()), _tptr(out_ptr), _tptr(out_idx), _tptr(out_x),
                                                _tptr(ws), int(ws.numel() * ws.element_size())))

    def csc_workspace(self, G: int, n_cells: int, nnz: int) -> dict:
        """Pre-allocated outputs / scratch of the GF-ICF pipeline (keeps allocation out of timed loops)."""
        tc, dev = self.torch, f"cuda:{self.device}"
        return dict(
            nt=tc.zeros(max(G, 1), dtype=tc.int64, device=dev),
            keep=tc.zeros(max(G, 1), dtype=tc.uint8, device=dev),
            genes=tc.zeros(genes_words(G), dtype=tc.float64, device=dev),   # opaque per-gene tables
            w=tc.zeros(max(G, 1), dtype=tc.float64, device=dev),
            gkept=tc.zeros(1, dtype=tc.int64, device=dev),
            out_colptr=tc.zeros(n_cells + 1, dtype=tc.int64, device=dev),
            out_rowidx=tc.zeros(max(nnz, 1), dtype=tc.int32, device=dev),
            out_x=tc.zeros(max(nnz, 1), dtype=tc.float64, device=dev),
        )

    def gficf_csc(self, G, N, colptr, rowidx, x, prop_min=0.05, prop_max=1.0, w_in=None, ws=None, exact: bool = False,
                  auto_exact: bool = False) -> dict:
        """Single-GPU GF-ICF on a device-resident CSC matrix (colptr int64).  Returns the workspace dict;
        ``out_colptr[N]`` is the kept nnz, ``gkept[0]`` the number of kept genes.

        ``exact=False``: the count pass does not read ``x`` (stored entries are taken for non-zero cells); if the matrix
        stores explicit zeros the next :meth:`sync` raises ``GFICF_ERR_EXPLICIT_ZEROS`` and the call is to be repeated
        with ``exact=True`` (the count pass reads ``x``: ``rowSums(M != 0)``, reference R/gficf.R:40,88).
        ``auto_exact=True`` does that here: the call synchronises, and if — and only if — the deferred status is
        ``GFICF_ERR_EXPLICIT_ZEROS`` the exact form runs in its place (any other deferred error of the same sync has
        precedence in ``gficf_ctx_sync`` and propagates); what returns is then complete and checked.  A caller that keeps
        the pass asynchronous (the bench's timed loop) leaves it off and owes the sync + retry itself."""
        ws = ws or self.csc_workspace(G, N, int(rowidx.numel()))

        def run(fn):
            check(fn(self._bind(), G, N, _tptr(colptr), _tptr(rowidx), _tptr(x), int(rowidx.numel()),
                     float(prop_min), float(prop_max), _tptr(w_in), _tptr(ws["nt"]),
                     _tptr(ws["keep"]), _tptr(ws["genes"]), _tptr(ws["w"]), _tptr(ws["gkept"]),
                     _tptr(ws["out_colptr"]), _tptr(ws["out_rowidx"]), _tptr(ws["out_x"])))

        run(self.L.gficf_csc_exact_device if exact else self.L.gficf_csc_device)
        if auto_exact:
            try:
                self.sync()
            except GficfError as ex:
                if exact or ex.code != 9:                       # 9 = GFICF_ERR_EXPLICIT_ZEROS
                    raise
                run(self.L.gficf_csc_exact_device)
                self.sync()
        return ws
