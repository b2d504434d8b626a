"""Builds tests/helpers/prim_probe.hip against gficf_amd/csrc/common.h into tests/helpers/libprim_probe.so (linked to
libgficf_hip.so) and binds it with ctypes: the radix sort, the int64 exclusive scan and the scan epoch of a context, which
the library keeps internal (the exported gficf_* surface is pinned by tests/test_abi.py), and the header-only code the add-ons
share (block_ops.h, addon_sort.h): the grouped f64 sort, the block sum and max, the LDS sort, the lower bound and the capped
grid; and what louvain.hip and leiden.hip share (community_ops.h): the numbering by size and the table insert.  Test
infrastructure only."""
from __future__ import annotations

import ctypes
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.join(ROOT, "tests", "helpers")
SRC = os.path.join(HERE, "prim_probe.hip")
SO = os.path.join(HERE, "libprim_probe.so")
LIBDIR = os.path.join(ROOT, "gficf_amd")
CSRC = os.path.join(LIBDIR, "csrc")
HEADERS = [os.path.join(CSRC, "common.h"), os.path.join(CSRC, "block_ops.h"), os.path.join(CSRC, "addon_sort.h"),
           os.path.join(CSRC, "community_ops.h"), os.path.join(ROOT, "include", "gficf_hip.h")]

SYMBOLS = ["probe_radix_sort_kv", "probe_radix_sort_hist_len", "probe_exclusive_scan_i64", "probe_get_scan_epoch",
           "probe_set_scan_epoch", "probe_ctx_sync", "probe_sort_f64", "probe_block_ops", "probe_lds_sort_u64",
           "probe_lower_bound_f64", "probe_lower_bound_u32", "probe_comm_number", "probe_comm_insert", "probe_grid_capped",
           "probe_grid_1d"]


def hipcc() -> str | None:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


def build(force: bool = False) -> str:
    """Compile the probe (gfx950) unless an up-to-date build is there; returns the path of the shared object."""
    cc = hipcc()
    if cc is None:
        raise RuntimeError("hipcc not found")
    lib = os.path.join(LIBDIR, "libgficf_hip.so")
    if not os.path.exists(lib):
        raise RuntimeError("gficf_amd/libgficf_hip.so is missing: run __graft_entry__.build() first")
    newest = max(os.path.getmtime(f) for f in [SRC, lib] + HEADERS)
    if force or not os.path.exists(SO) or os.path.getmtime(SO) < newest:
        tmp = SO + ".tmp%d" % os.getpid()
        cmd = [cc, "-O2", "-std=c++17", "--offload-arch=gfx950", "-shared", "-fPIC", "-Wall", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
               SRC, "-L", LIBDIR, "-lgficf_hip", "-Wl,-rpath," + LIBDIR, "-o", tmp]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError("building the primitive probe failed:\n" + r.stderr[-3000:])
        os.replace(tmp, SO)
    return SO


class Probe:
    def __init__(self):
        import torch  # noqa: F401  (one HIP runtime in the process, as gficf_amd/_lib.py has it)

        from gficf_amd import _lib

        _lib.load()
        self.L = L = ctypes.CDLL(build())
        vp, i64, ci, u32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_uint32
        for name, res, args in [
            ("probe_radix_sort_kv", ci, [vp, vp, vp, vp, i64, ci, vp, vp]),
            ("probe_radix_sort_hist_len", i64, [i64, ci]),
            ("probe_exclusive_scan_i64", ci, [vp, vp, i64]),
            ("probe_get_scan_epoch", u32, [vp]),
            ("probe_set_scan_epoch", None, [vp, u32]),
            ("probe_ctx_sync", ci, [vp]),
            ("probe_sort_f64", ci, [vp, vp, i64, vp, ci, vp, vp, u32, vp, vp, u32, ci, ctypes.POINTER(i64), ctypes.POINTER(i64)]),
            ("probe_block_ops", ci, [vp, vp, vp, i64, vp]),
            ("probe_lds_sort_u64", ci, [vp, vp, ci, i64]),
            ("probe_lower_bound_f64", ci, [vp, vp, i64, vp, i64, vp]),
            ("probe_lower_bound_u32", ci, [vp, vp, ci, vp, i64, vp]),
            ("probe_comm_number", ci, [vp, vp, i64, i64, vp, vp, vp, vp, ctypes.POINTER(i64), ctypes.POINTER(i64)]),
            ("probe_comm_insert", ci, [vp, ci, vp, vp, vp, vp, vp, vp]),
            ("probe_grid_capped", ctypes.c_uint, [i64, i64, ctypes.c_uint]),
            ("probe_grid_1d", ctypes.c_uint, [i64]),
        ]:
            f = getattr(L, name)
            f.restype, f.argtypes = res, args

    def sort_kv(self, ctx, kv0, kv1, hist, M, b, okey, oval) -> int:
        return self.L.probe_radix_sort_kv(ctx, kv0, kv1, hist, int(M), int(b), okey, oval)

    def hist_len(self, M, b) -> int:
        return int(self.L.probe_radix_sort_hist_len(int(M), int(b)))

    def scan(self, ctx, d, n) -> int:
        return self.L.probe_exclusive_scan_i64(ctx, d, int(n))

    def epoch(self, ctx) -> int:
        return int(self.L.probe_get_scan_epoch(ctx))

    def set_epoch(self, ctx, e: int):
        self.L.probe_set_scan_epoch(ctx, int(e))

    def sync(self, ctx) -> int:
        return self.L.probe_ctx_sync(ctx)

    def sort_f64_bytes(self, n, group_bits) -> int:
        """The block gficf_sort_bufs::take asks for: n elements, one group width (0: none)."""
        total = ctypes.c_int64(0)
        assert self.L.probe_sort_f64(None, None, int(n), None, 0, None, None, 0, None, None, 0, int(group_bits), None, ctypes.byref(total)) == 0
        return total.value

    def sort_f64(self, ctx, ws, n, v, desc, mask, status, st_bit, count, group, G, group_bits):
        """Enqueues the sort; returns (rc, the byte offsets of key, kv0, kv1, hist, okey, oval in ws)."""
        offs, total = (ctypes.c_int64 * 6)(), ctypes.c_int64(0)
        rc = self.L.probe_sort_f64(ctx, ws, int(n), v, int(desc), mask, status, int(st_bit), count, group, int(G), int(group_bits), offs,
                                   ctypes.byref(total))
        return rc, list(offs)

    def block_ops(self, ctx, a, b, nblocks, out) -> int:
        return self.L.probe_block_ops(ctx, a, b, int(nblocks), out)

    def lds_sort(self, ctx, data, np2, nblocks) -> int:
        return self.L.probe_lds_sort_u64(ctx, data, int(np2), int(nblocks))

    def lower_f64(self, ctx, a, n, q, m, out) -> int:
        return self.L.probe_lower_bound_f64(ctx, a, int(n), q, int(m), out)

    def lower_u32(self, ctx, a, n, q, m, out) -> int:
        return self.L.probe_lower_bound_u32(ctx, a, int(n), q, int(m), out)

    def comm_number_bytes(self, N) -> int:
        """The block gficf_comm_sort_bufs::take asks for, for N vertices."""
        total = ctypes.c_int64(0)
        assert self.L.probe_comm_number(None, None, 0, int(N), None, None, None, None, None, ctypes.byref(total)) == 0
        return total.value

    def comm_number(self, ctx, ws, C, N, cnt, lab, rank, out):
        """Enqueues the numbering; returns (rc, the byte offsets of kv[0], kv[1], key, id, hist in ws)."""
        offs, total = (ctypes.c_int64 * 5)(), ctypes.c_int64(0)
        rc = self.L.probe_comm_number(ctx, ws, int(C), int(N), cnt, lab, rank, out, offs, ctypes.byref(total))
        return rc, list(offs)

    def comm_insert(self, ctx, rounds, c, w, slot, own, key_out, val_out) -> int:
        return self.L.probe_comm_insert(ctx, int(rounds), c, w, slot, own, key_out, val_out)

    def grid_capped(self, n, per, cap) -> int:
        return int(self.L.probe_grid_capped(int(n), int(per), int(cap)))

    def grid_1d(self, n) -> int:
        return int(self.L.probe_grid_1d(int(n)))
