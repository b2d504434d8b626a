"""GPU: the library's shared primitives on their own, at the sizes where their branches switch.

  radix sort   gficf_radix_sort_kv (radix_sort.hip): 1..4 passes, uneven last pass, workgroups walking several tiles
               (M > 768 * 4096), stability, key bits above b ignored, nothing written past hist / okey / oval
  scan         gficf_exclusive_scan_i64 (ctx.hip): tile edges, the largest n the look-back workspace takes and one tile
               beyond, the 2^40 value limit, scans queued back to back, the epoch wrap at 2^22
  transpose    gficf_csc_transpose (transpose.hip): pairing (G <= 9000), plain with one gene range and with several
               (G > 36864), the cells-per-block floor of 16 and cap of 1024, long cells, empty cells and genes, explicit zeros

  f64 sort     gficf_sort_f64 (addon_sort.h): the add-ons' stable sort of doubles within groups against numpy.lexsort, every
               form of its first pass (descending, mask, status, count) and of its groups (none, array, divisor), the
               buffers carved by gficf_sort_bufs::take, nothing written outside them
  block ops    block_ops.h: the folded sum and max against the same tree in NumPy, bit for bit; the LDS sort; the lower bound
               and the capped grid
  communities  community_ops.h: the numbering of labels by decreasing size against a NumPy stable sort by (-size, id), and the
               LDS table insert of one wave (owners, exact sums, a full table)

The sort, the scan and the add-ons' headers are reached through tests/helpers/prim_probe.py; references are exact (NumPy /
torch stable sorts, integer cumulative sums, the same float64 additions in the same order)."""
import numpy as np
import pytest
import scipy.sparse as sp

import gficf_amd
from gficf_amd.api import default_context
from tests.helpers import prim_probe

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
RS_TILE, RS_MAX_WGS = 4096, 768
BIG = RS_TILE * RS_MAX_WGS                                 # 3,145,728: beyond it a workgroup walks several tiles
SCAN_TILE, SCAN_MAX_TILES = 4096, 131071                   # 1 MiB look-back workspace: ticket word + 131,071 descriptors
CANARY = 0x5A5A5A5A
OK, INVALID_ARG, BAD_CSC, UNSUPPORTED = 0, 1, 3, 6
B_ALL = [1, 2, 7, 8, 9, 10, 11, 17, 20, 21, 31, 32]


@pytest.fixture(scope="module")
def probe():
    if prim_probe.hipcc() is None:
        pytest.skip("hipcc not available")
    return prim_probe.Probe()


@pytest.fixture(scope="module")
def ctx():
    c = default_context()
    c.sync()
    return c.handle


def _ptr(t):
    return None if t is None else t.data_ptr()


def _i32(u):
    """uint32 bit patterns held in int64 -> int32 tensor of the same bits."""
    return (u - (u >= 2 ** 31).to(torch.int64) * 2 ** 32).to(torch.int32)


def _padded(n, canary, dtype):
    return torch.full((n + 64,), canary, dtype=dtype, device=DEV)


# ------------------------------------------------------------------------------------------------ radix sort
def _keys(kind, M, b, gen):
    """uint32 keys (in int64) of one kind; the sort looks at their low b bits only."""
    mask = (1 << b) - 1
    if kind == "uniform":
        return torch.randint(0, mask + 1, (M,), generator=gen, device=DEV, dtype=torch.int64)
    if kind == "equal":
        return torch.full((M,), 0x9E3779B9 & mask, dtype=torch.int64, device=DEV)
    if kind == "two":
        return torch.where(torch.rand(M, generator=gen, device=DEV) < 0.5, 0, mask).to(torch.int64)
    if kind in ("ascending", "descending"):
        k = torch.sort(torch.randint(0, mask + 1, (M,), generator=gen, device=DEV, dtype=torch.int64)).values
        return k if kind == "ascending" else k.flip(0)
    if kind == "highbits":                                  # every key carries random bits above b: ignored by the sort
        return torch.randint(0, 2 ** 32, (M,), generator=gen, device=DEV, dtype=torch.int64)
    raise ValueError(kind)


def _values(kind, M, gen):
    if kind == "index":                                     # the element's own position: stability is visible
        return torch.arange(M, dtype=torch.int64, device=DEV)
    v = torch.randint(0, 2 ** 32, (M,), generator=gen, device=DEV, dtype=torch.int64)
    v[M // 2] = 0xFFFFFFFF
    v[0] = 0
    return v


def _sort_and_check(probe, ctx, key, val, b):
    M = key.numel()
    hl = probe.hist_len(M, b)
    kv0 = _padded(M, CANARY, torch.int64)
    words = kv0[:M].view(torch.int32).view(M, 2)           # element = key << 32 | value, little-endian words
    words[:, 0], words[:, 1] = _i32(val), _i32(key)
    kv1 = _padded(M, CANARY, torch.int64)
    hist = _padded(hl, CANARY, torch.int64)
    okey = _padded(M, CANARY, torch.int32)
    oval = _padded(M, CANARY, torch.int32)
    torch.cuda.synchronize()
    assert probe.sort_kv(ctx, _ptr(kv0), _ptr(kv1), _ptr(hist), M, b, _ptr(okey), _ptr(oval)) == OK
    assert probe.sync(ctx) == OK
    order = torch.sort(key & ((1 << b) - 1), stable=True).indices
    assert torch.equal(okey[:M], _i32(key[order])), (M, b)          # the full 32-bit key, not the masked one
    assert torch.equal(oval[:M], _i32(val[order])), (M, b)
    for t in (hist[hl:], okey[M:], oval[M:], kv0[M:], kv1[M:]):
        assert bool((t == CANARY).all()), (M, b)


@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 4095, 4096, 4097])
def test_radix_sort_small_every_width_and_key_kind(probe, ctx, M):
    gen = torch.Generator(device=DEV).manual_seed(M)
    for b in B_ALL:
        for kind in ("uniform", "equal", "two", "ascending", "descending", "highbits"):
            for vk in ("index", "random"):
                _sort_and_check(probe, ctx, _keys(kind, M, b, gen), _values(vk, M, gen), b)


@pytest.mark.parametrize("M", [BIG - 1, BIG, BIG + 1, 2 * BIG + 4097, 20_000_003])
def test_radix_sort_tiles_walked_by_each_workgroup(probe, ctx, M):
    """Past 768 tiles every workgroup walks ceil(tiles / 768) of them and carries its digits' places from tile to tile."""
    gen = torch.Generator(device=DEV).manual_seed(M)
    for b in B_ALL:
        _sort_and_check(probe, ctx, _keys("highbits" if b in (9, 21, 31) else "uniform", M, b, gen), _values("index", M, gen), b)
    for kind in ("equal", "two", "descending"):             # one digit fills every tile / two runs / a reversed run
        _sort_and_check(probe, ctx, _keys(kind, M, 32, gen), _values("random", M, gen), 32)
    _sort_and_check(probe, ctx, _keys("ascending", M, 18, gen), _values("index", M, gen), 18)


def test_radix_sort_argument_errors_write_nothing(probe, ctx):
    M = 1000
    kv0 = _padded(M, CANARY, torch.int64)
    kv1 = _padded(M, CANARY, torch.int64)
    hist = _padded(probe.hist_len(M, 32), CANARY, torch.int64)
    okey = _padded(M, CANARY, torch.int32)
    oval = _padded(M, CANARY, torch.int32)
    bufs = (kv0, kv1, hist, okey, oval)
    torch.cuda.synchronize()
    assert probe.sort_kv(ctx, *map(_ptr, (kv0, kv1, hist)), 0, 32, _ptr(okey), _ptr(oval)) == OK      # M = 0: nothing launched
    for b in (0, 33, -1):
        assert probe.sort_kv(ctx, *map(_ptr, (kv0, kv1, hist)), M, b, _ptr(okey), _ptr(oval)) == INVALID_ARG
    for m in (2 ** 32, 2 ** 40, -1):                        # validated before any pointer is used
        assert probe.sort_kv(ctx, None, None, None, m, 32, None, None) == INVALID_ARG
    assert probe.sync(ctx) == OK
    for t in bufs:
        assert bool((t == CANARY).all())


# ------------------------------------------------------------------------------------------------ scan
def _scan_and_check(probe, ctx, d, total_ok=True):
    want = torch.cumsum(d, 0) - d
    got = d.clone()
    torch.cuda.synchronize()
    assert probe.scan(ctx, _ptr(got), got.numel()) == OK
    assert probe.sync(ctx) == (OK if total_ok else BAD_CSC)
    if total_ok:
        assert torch.equal(got, want), got.numel()


@pytest.mark.parametrize("n", [1, 2, 4095, 4096, 4097, 3 * 4096 + 1, 10_000_003])
def test_scan_tile_edges(probe, ctx, n):
    gen = torch.Generator(device=DEV).manual_seed(n)
    d = torch.randint(0, 1000, (n,), generator=gen, device=DEV, dtype=torch.int64)
    _scan_and_check(probe, ctx, d)
    d[2::3] = -d[2::3] // 3                                 # negative elements, non-negative tile totals
    if n >= 3:
        _scan_and_check(probe, ctx, d)


def test_scan_largest_workspace_and_one_tile_beyond(probe, ctx):
    n = SCAN_MAX_TILES * SCAN_TILE                          # 536,866,816 elements: every descriptor of the workspace
    d = torch.empty(n + 1, dtype=torch.int64, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(3)
    d.random_(0, 4, generator=gen)
    want = torch.cumsum(d[:n], 0)
    want -= d[:n]
    torch.cuda.synchronize()
    assert probe.scan(ctx, _ptr(d), n) == OK
    assert probe.sync(ctx) == OK
    assert torch.equal(d[:n], want)
    del want
    before = d[n].item()
    epoch = probe.epoch(ctx)
    assert probe.scan(ctx, _ptr(d), n + 1) == UNSUPPORTED  # tile 131,072 has no descriptor
    assert probe.epoch(ctx) == epoch and probe.sync(ctx) == OK and d[n].item() == before
    assert "exceed the look-back workspace" in gficf_amd._lib.last_error()


def test_scan_value_limit_two_to_the_forty(probe, ctx):
    lim = 1 << 40
    # one tile: the total just below the limit is exact, the limit itself and a negative total are reported at the sync
    d = torch.zeros(4000, dtype=torch.int64, device=DEV)
    d[0], d[1], d[3999] = lim // 2, lim // 2 - 2, 1
    _scan_and_check(probe, ctx, d)
    d[3999] = 2
    _scan_and_check(probe, ctx, d, total_ok=False)
    d = torch.ones(5000, dtype=torch.int64, device=DEV)
    d[4500] = -10_000
    _scan_and_check(probe, ctx, d, total_ok=False)
    # several tiles, every tile's own total below the limit: the running prefix carries it
    n = 8 * SCAN_TILE
    d = torch.zeros(n, dtype=torch.int64, device=DEV)
    d[::SCAN_TILE] = lim // 8
    d[0] -= 1
    _scan_and_check(probe, ctx, d)                          # total 2^40 - 1: exact
    d[0] += 1
    _scan_and_check(probe, ctx, d, total_ok=False)          # total 2^40: reported, not wrapped into 40 bits
    assert probe.sync(ctx) == OK                            # the flag was taken by the previous sync


def test_scans_queued_back_to_back(probe, ctx):
    gen = torch.Generator(device=DEV).manual_seed(5)
    sizes = [5000, 1, 1_000_007, 4096, 300_001, 4097, 2]
    data = [torch.randint(-50, 1000, (n,), generator=gen, device=DEV, dtype=torch.int64).abs() for n in sizes]
    want = [torch.cumsum(d, 0) - d for d in data]
    torch.cuda.synchronize()
    for d in data:
        assert probe.scan(ctx, _ptr(d), d.numel()) == OK
    assert probe.sync(ctx) == OK
    for d, w in zip(data, want):
        assert torch.equal(d, w)


def test_scan_epoch_wrap(probe, ctx):
    """The look-back descriptors carry a 22-bit epoch; at 2^22 the workspace is cleared and the count starts over at 1."""
    assert probe.sync(ctx) == OK
    probe.set_epoch(ctx, (1 << 22) - 3)
    gen = torch.Generator(device=DEV).manual_seed(6)
    sizes = [50_000, 123_457, 4 * 4096 + 17, 200_000, 9000, 70_001]
    data = [torch.randint(0, 10_000, (n,), generator=gen, device=DEV, dtype=torch.int64) for n in sizes]
    want = [torch.cumsum(d, 0) - d for d in data]
    epochs = []
    torch.cuda.synchronize()
    for d in data:
        assert probe.scan(ctx, _ptr(d), d.numel()) == OK
        epochs.append(probe.epoch(ctx))
    assert probe.sync(ctx) == OK
    assert epochs == [(1 << 22) - 2, (1 << 22) - 1, 1, 2, 3, 4]
    for d, w in zip(data, want):
        assert torch.equal(d, w)
    d = torch.ones(3 * SCAN_TILE, dtype=torch.int64, device=DEV)   # the context goes on working
    _scan_and_check(probe, ctx, d)


# ------------------------------------------------------------------------------------------------ transpose
def _random_csc(G, N, nnz, seed, long_cells=(), empty_cells=(), empty_genes=(), zeros_every=0):
    """genes x cells CSC with about nnz entries; long_cells get many entries each, the listed cells / genes none."""
    rng = np.random.default_rng(seed)
    cell = rng.integers(0, N, nnz, dtype=np.int64)
    gene = rng.integers(0, G, nnz, dtype=np.int64)
    for c, k in long_cells:
        cell = np.concatenate([cell, np.full(k, c)])
        gene = np.concatenate([gene, rng.choice(G, k, replace=False)])
    keep = ~np.isin(cell, list(empty_cells)) & ~np.isin(gene, list(empty_genes))
    lin = np.unique(cell[keep] * G + gene[keep])
    c, g = lin // G, lin % G
    colptr = np.zeros(N + 1, dtype=np.int64)
    np.add.at(colptr, c + 1, 1)
    colptr = np.cumsum(colptr)
    x = rng.integers(1, 50, len(lin)).astype(np.float64) + rng.random(len(lin))
    if zeros_every:
        x[::zeros_every] = 0.0
    return colptr, g.astype(np.int32), x


def _check_transpose(G, N, cp, ri, x, ops):
    from oracle import oracle_np

    ptr, idx, val = oracle_np.transpose_np(G, N, cp, ri, x)
    S = sp.csc_matrix((x, ri, cp), shape=(G, N)).T.tocsc()          # scipy's own transpose as a second opinion
    S.sort_indices()
    assert np.array_equal(S.indptr, ptr) and np.array_equal(S.indices, idx) and np.array_equal(S.data, val)
    # host entry
    T = gficf_amd.transpose_gficf(sp.csc_matrix((x, ri, cp), shape=(G, N)))
    assert np.array_equal(T.indptr, ptr) and np.array_equal(T.indices, idx) and np.array_equal(T.data, val)
    # device entry and the begin / end form (gaps between the columns of the input)
    nnz = len(ri)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    ws = torch.zeros(ops.csc_transpose_workspace_bytes(G, N), dtype=torch.uint8, device=DEV)
    o_ptr = torch.full((G + 1 + 16,), -7, dtype=torch.int64, device=DEV)
    o_idx = torch.full((nnz + 16,), -7, dtype=torch.int32, device=DEV)
    o_x = torch.full((nnz + 16,), -7.0, dtype=torch.float64, device=DEV)
    ops.csc_transpose(G, N, t(cp), t(ri), t(x), o_ptr, o_idx[:max(nnz, 1)], o_x[:max(nnz, 1)], ws)
    ops.sync()
    assert np.array_equal(o_ptr[:G + 1].cpu().numpy(), ptr) and np.array_equal(o_idx[:nnz].cpu().numpy(), idx)
    assert np.array_equal(o_x[:nnz].cpu().numpy(), val)
    assert bool((o_ptr[G + 1:] == -7).all()) and bool((o_idx[nnz:] == -7).all()) and bool((o_x[nnz:] == -7.0).all())
    gap = 3
    lens = np.diff(cp)
    beg = cp + gap * np.arange(N + 1)
    ri_b = np.full(nnz + gap * N, G + 5, dtype=np.int32)             # junk in the gaps: never read
    x_b = np.full(nnz + gap * N, np.nan)
    pos = np.repeat(beg[:-1], lens) + (np.arange(nnz) - np.repeat(cp[:-1], lens))
    ri_b[pos], x_b[pos] = ri, x
    o_ptr.fill_(-7)
    ops.csc_transpose_be(G, N, t(beg[:-1]), t(beg[:-1] + lens), t(ri_b), t(x_b), o_ptr, o_idx[:max(nnz, 1)], o_x[:max(nnz, 1)], ws)
    ops.sync()
    assert np.array_equal(o_ptr[:G + 1].cpu().numpy(), ptr) and np.array_equal(o_idx[:nnz].cpu().numpy(), idx)
    assert np.array_equal(o_x[:nnz].cpu().numpy(), val)


@pytest.mark.parametrize("G", [9000, 9001, 23000, 36864, 36865, 73729])
def test_transpose_forms_at_their_gene_edges(G):
    """9000 / 9001: pairing / plain; 23000: plain, one gene range; 36864 / 36865: one / two ranges; 73729: three.
    N = 300 cells: 16 cells a block (the floor) in either form.  Long cells, empty cells and genes, explicit zeros."""
    ops = gficf_amd.HipOps(0)
    N = 300
    cp, ri, x = _random_csc(G, N, 60_000, seed=G, long_cells=[(7, min(G, 5000)), (299, 1500)], empty_cells=(0, 150, 151),
                            empty_genes=(0, G // 2, G - 1), zeros_every=13)
    assert np.diff(cp)[7] > 1024 and np.diff(cp)[0] == 0
    _check_transpose(G, N, cp, ri, x, ops)


@pytest.mark.parametrize("G,N", [(9000, 270_000), (23000, 800_000), (40000, 790_000)])
def test_transpose_cells_per_block_cap(G, N):
    """Pairing beyond 256 * 1024 cells and plain beyond 768 * 1024: 1024 cells a block, more blocks than the cap implies."""
    ops = gficf_amd.HipOps(0)
    cp, ri, x = _random_csc(G, N, 2_500_000, seed=N, long_cells=[(N - 1, 3000), (N // 2, 1100)], empty_cells=(1, 2, N - 2),
                            empty_genes=(5,), zeros_every=29)
    _check_transpose(G, N, cp, ri, x, ops)


# ------------------------------------------------------------------------------------------------ what the add-ons share
# block_ops.h and addon_sort.h are header-only: the probe compiles them as the add-ons do.
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bit_width(n):
    """gficf_bit_width: the smallest b in 1..32 with 2^b > n."""
    return max(1, int(n).bit_length())


def _sort_values(n, rng, inf=True):
    """n doubles without a NaN: both zeros, both infinities, denormals, many exact duplicates, pairs whose keys differ in the
    low 32 bits only and pairs whose keys differ in the high 32 bits only (what a dropped or swapped pass gets wrong)."""
    base = rng.standard_normal(24) * 10.0 ** rng.integers(-6, 7, 24)
    bits = base.view(np.uint64)
    hi, lo = bits >> np.uint64(32), rng.integers(0, 2 ** 32, 24, dtype=np.uint64)
    low_pairs = np.concatenate([(hi << np.uint64(32)) | lo, (hi << np.uint64(32)) | (lo ^ np.uint64(0x80000001))]).view(np.float64)
    high_pairs = np.concatenate([(hi << np.uint64(32)) | lo[0], (np.roll(hi, 1) << np.uint64(32)) | lo[0]]).view(np.float64)
    special = [0.0, -0.0, 5e-324, -5e-324, 1.1e-308, -3.3e-310, 1.7976931348623157e308] + ([np.inf, -np.inf] if inf else [])
    first = [0, 24, 1, 25, 2, 26]                           # three pairs of either kind ahead, for the smallest n
    pool = np.concatenate([np.array(special), low_pairs[first], high_pairs[first], low_pairs, high_pairs, base[:6], -base[:6]])
    assert not np.isnan(pool).any()
    if n < 8:
        return rng.choice(np.array(special), n)
    body = np.concatenate([pool, rng.choice(pool, max(n - 4 - len(pool), 0))])[:n - 4]
    if n > 600:
        body[len(pool)::3] = rng.standard_normal(len(body[len(pool)::3]))     # distinct values among the duplicates
    return np.concatenate([[0.0, -0.0, -0.0, 0.0], rng.permutation(body)])    # the zeros must tie and keep this order


def _expected_order(v, desc, mask, group):
    """numpy.lexsort on (group, masked-out last, value, original position); -0.0 is +0.0, a masked-out value does not count."""
    x = v + 0.0 if mask is None else np.where(mask != 0, v + 0.0, 0.0)
    keys = [np.arange(len(v)), -x if desc else x]
    keys.append(np.zeros(len(v), dtype=np.int8) if mask is None else (mask == 0).astype(np.int8))
    keys.append(np.zeros(len(v), dtype=np.int64) if group is None else group.astype(np.int64))
    return np.lexsort(tuple(keys))


def _f64_sort_and_check(probe, ctx, v, desc, mask=None, group=None, G=0, group_bits=0, status_bit=0, want_status=0):
    n = len(v)
    total = probe.sort_f64_bytes(n, group_bits)
    ws = torch.full((total,), 0x5A, dtype=torch.uint8, device=DEV)
    d_v, d_mask = _dev(v), None if mask is None else _dev(mask.astype(np.int32))
    d_group = None if group is None or G else _dev(group.astype(np.uint32).view(np.int32))
    status = torch.tensor([0, CANARY], dtype=torch.int32, device=DEV)
    count = torch.tensor([0, CANARY], dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    rc, offs = probe.sort_f64(ctx, _ptr(ws), n, _ptr(d_v), desc, _ptr(d_mask), _ptr(status) if status_bit else None, status_bit, _ptr(count),
                              _ptr(d_group), G, group_bits)
    assert rc == OK and probe.sync(ctx) == OK
    order = _expected_order(v, desc, mask, group)
    o_key, _, _, o_hist, o_okey, o_oval = offs
    oval = ws[o_oval:o_oval + 4 * n].view(torch.int32).cpu().numpy().view(np.uint32)
    assert np.array_equal(oval, order.astype(np.uint32)), (n, desc, group_bits)
    if group is not None:
        okey = ws[o_okey:o_okey + 4 * n].view(torch.int32).cpu().numpy().view(np.uint32)
        assert np.array_equal(okey, group[order].astype(np.uint32)), (n, desc, group_bits)
    key = ws[o_key:o_key + 8 * n].view(torch.int64).cpu().numpy().view(np.uint64)
    kept = np.ones(n, dtype=bool) if mask is None else mask != 0
    assert (key[~kept] == np.uint64(2 ** 64 - 1)).all() and (key[kept] != np.uint64(2 ** 64 - 1)).all()
    assert count.tolist() == [int(kept.sum()), CANARY] and status.tolist() == [want_status, CANARY]
    assert np.array_equal(d_v.cpu().numpy().view(np.uint64), v.view(np.uint64))            # the input is left alone
    # nothing written outside the six buffers: n elements each (the + 1 of kv0 / kv1 is not the sort's), the histogram as
    # long as the widest pass asks
    hl = max(probe.hist_len(n, 32), probe.hist_len(n, group_bits) if group_bits else 0)
    used = torch.zeros(total, dtype=torch.bool, device=DEV)
    for off, size in zip(offs, (8 * n, 8 * n, 8 * n, 8 * hl, 4 * n, 4 * n)):
        assert off % 256 == 0 and off + size <= total
        used[off:off + size] = True
    assert bool((ws[~used] == 0x5A).all()), (n, desc, group_bits)


SORT_N = [1, 2, 255, 256, 257, 4096, 4097, 70_001]


@pytest.mark.parametrize("n", SORT_N)
def test_f64_sort_against_lexsort(probe, ctx, n):
    """Ascending and descending; no group and group by array, its width as markers.hip computes it (gficf_bit_width(G))."""
    rng = np.random.default_rng(n)
    v = _sort_values(n, rng)
    Gn = max(1, n // 14)                                    # 70 001: 5000 groups, 13 bits, two digit passes
    group = rng.integers(0, Gn, n)
    for desc in (0, 1):
        _f64_sort_and_check(probe, ctx, v, desc)
        _f64_sort_and_check(probe, ctx, v, desc, group=group, group_bits=_bit_width(Gn))


@pytest.mark.parametrize("C", [1, 5])
def test_f64_sort_group_by_divisor(probe, ctx, C):
    """n = G C statistics, entry p in group p / G, G = 37: the width as gsea.hip and gsva.hip compute it (gficf_bit_width(C - 1))."""
    G = 37
    rng = np.random.default_rng(100 + C)
    v = _sort_values(G * C, rng)
    group = np.arange(G * C) // G
    mask = (rng.random(G * C) < 0.7).astype(np.int32)
    for desc in (0, 1):
        _f64_sort_and_check(probe, ctx, v, desc, group=group, G=G, group_bits=_bit_width(C - 1))
        _f64_sort_and_check(probe, ctx, v, desc, mask=mask, group=group, G=G, group_bits=_bit_width(C - 1))


@pytest.mark.parametrize("n", SORT_N)
def test_f64_sort_mask_status_count(probe, ctx, n):
    """Masked-out entries come last in input order (within their group) and are not counted; one infinity raises the status
    bit and the order is still right; an infinity that is masked out is not looked at."""
    rng = np.random.default_rng(1000 + n)
    v = _sort_values(n, rng, inf=False)
    mask = (rng.random(n) < 0.6).astype(np.int32)
    group = rng.integers(0, 3, n)
    for desc in (0, 1):
        _f64_sort_and_check(probe, ctx, v, desc, mask=mask, status_bit=4, want_status=0)
        _f64_sort_and_check(probe, ctx, v, desc, mask=mask, group=group, group_bits=_bit_width(3), status_bit=4, want_status=0)
    w = v.copy()
    w[n // 2] = np.inf
    m = mask.copy()
    m[n // 2] = 1
    _f64_sort_and_check(probe, ctx, w, 0, status_bit=4, want_status=4)
    _f64_sort_and_check(probe, ctx, w, 1, mask=m, status_bit=2, want_status=2)
    m[n // 2] = 0
    _f64_sort_and_check(probe, ctx, w, 1, mask=m, status_bit=2, want_status=0)


def test_block_sum_and_max_are_the_fixed_tree(probe, ctx):
    """256 partials over 30 orders of magnitude with mixed signs: any other order of the additions gives other bits.  Sum and
    max, each twice back to back through one LDS buffer, in 300 workgroups."""
    nb = 300
    rng = np.random.default_rng(7)
    a, b = (rng.choice([-1.0, 1.0], (nb, 256)) * 10.0 ** rng.uniform(-15, 15, (nb, 256)) for _ in range(2))
    out = torch.full((4 * nb + 16,), -7.0, dtype=torch.float64, device=DEV)
    d_a, d_b = _dev(a), _dev(b)
    torch.cuda.synchronize()
    assert probe.block_ops(ctx, _ptr(d_a), _ptr(d_b), nb, _ptr(out)) == OK and probe.sync(ctx) == OK

    def tree(x):
        s = x.copy()
        h = 128
        while h >= 1:
            s[:, :h] = s[:, :h] + s[:, h:2 * h]
            h >>= 1
        return s[:, 0]

    got = out[:4 * nb].cpu().numpy().reshape(nb, 4)
    for j, want in enumerate((tree(a), tree(b), a.max(axis=1), b.max(axis=1))):
        assert np.array_equal(got[:, j].view(np.uint64), want.view(np.uint64)), j
    assert (np.sort(a, axis=1).sum(axis=1) != tree(a)).any()           # the inputs do tell the orders apart
    assert bool((out[4 * nb:] == -7.0).all())


@pytest.mark.parametrize("np2", [2, 64, 256, 512, 2048, 8192])
def test_lds_sort_u64(probe, ctx, np2):
    nb = 5
    rng = np.random.default_rng(np2)
    x = rng.integers(0, 2 ** 64, (nb, np2), dtype=np.uint64)
    x[:, ::3] = rng.choice(x[0, :4], x[:, ::3].shape)       # duplicates
    x[1, np2 // 2:] = np.uint64(2 ** 64 - 1)                # the padding the callers add
    x[2, 1:] = np.uint64(2 ** 64 - 1)
    x[3] = np.sort(x[3])[::-1]
    d = torch.cat([_dev(x.view(np.int64)).reshape(-1), torch.full((64,), CANARY, dtype=torch.int64, device=DEV)])
    torch.cuda.synchronize()
    assert probe.lds_sort(ctx, _ptr(d), np2, nb) == OK and probe.sync(ctx) == OK
    got = d[:nb * np2].cpu().numpy().view(np.uint64).reshape(nb, np2)
    assert np.array_equal(got, np.sort(x, axis=1))
    assert bool((d[nb * np2:] == CANARY).all())


@pytest.mark.parametrize("n", [0, 1, 2, 1000])
def test_lower_bound(probe, ctx, n):
    """double / int64 and uint32 / int: below the first, above the last, at and next to every distinct value."""
    rng = np.random.default_rng(n + 11)
    a64 = np.sort(rng.choice(rng.standard_normal(max(n // 3, 1)) * 100.0, n))              # duplicates
    a32 = np.sort(rng.choice(rng.integers(1, 2 ** 32 - 1, max(n // 3, 1), dtype=np.uint32), n))   # both halves of the range
    for a, lower, one in ((a64, probe.lower_f64, None), (a32, probe.lower_u32, np.uint32(1))):
        d = np.unique(a)
        if one is None:
            q = np.concatenate([d, np.nextafter(d, -np.inf), np.nextafter(d, np.inf), [-1e300, 1e300, 0.0]])
            out = torch.full((len(q) + 16,), -7, dtype=torch.int64, device=DEV)
            d_a, d_q = _dev(a), _dev(q)
        else:
            q = np.concatenate([d, d - one, d + one, np.array([0, 2 ** 32 - 1], dtype=np.uint32)]).astype(np.uint32)
            out = torch.full((len(q) + 16,), -7, dtype=torch.int32, device=DEV)
            d_a, d_q = _dev(a.view(np.int32)), _dev(q.view(np.int32))
        torch.cuda.synchronize()
        assert lower(ctx, _ptr(d_a), n, _ptr(d_q), len(q), _ptr(out)) == OK and probe.sync(ctx) == OK
        assert np.array_equal(out[:len(q)].cpu().numpy(), np.searchsorted(a, q, side="left"))
        assert bool((out[len(q):] == -7).all())


def test_grid_capped_on_the_host(probe):
    """n = 0, 1, per, per + 1 and beyond the cap; gficf_grid_1d is the same helper at 256 a workgroup, capped at 16384."""
    for per, cap in ((256, 16384), (4, 1536), (2, 1280), (1, 1280), (256, 1 << 30)):
        want = [1, 1, 1, 2, cap]
        got = [probe.grid_capped(n, per, cap) for n in (0, 1, per, per + 1, per * cap + 1)]
        assert got == want, (per, cap, got)
        assert probe.grid_capped(per * cap, per, cap) == cap and probe.grid_capped(per * (cap - 1) + 1, per, cap) == cap
    for n in (0, 1, 256, 257, 256 * 16384 + 1):
        assert probe.grid_1d(n) == probe.grid_capped(n, 256, 16384)


# ------------------------------------------------------------------------------------------------ what Louvain and Leiden share
def _number_cases():
    rng = np.random.default_rng(5)
    sizes = np.zeros(257, dtype=np.int64)                   # a second workgroup of the C-sized kernels; unused labels (size 0)
    used = rng.choice(257, 180, replace=False)
    sizes[used] = 1
    np.add.at(sizes, rng.choice(used, 600 - 180), 1)        # many ties
    return {"C1": (np.array([7]), None), "C5_two_ties": (np.array([3, 5, 3, 1, 5]), None), "C257_N600_zeros": (sizes, None),
            "C300_singletons": (np.ones(300, dtype=np.int64), rng.permutation(300))}


NUMBER_CASES = _number_cases()


@pytest.mark.parametrize("case", sorted(NUMBER_CASES))
def test_number_by_size_against_stable_sort(probe, ctx, case):
    """rank = the position of a label in the stable sort by (-size, id) — a label nobody carries comes last, as Leiden's
    unused ones do — and out[v] = rank[lab[v]]; nothing written behind rank, out or outside the sort's buffers."""
    sizes, lab = NUMBER_CASES[case]
    C, N = len(sizes), int(sizes.sum())
    if lab is None:
        lab = np.random.default_rng(C).permutation(np.repeat(np.arange(C), sizes))
    assert len(lab) == N and np.array_equal(np.bincount(lab, minlength=C), sizes)
    order = np.lexsort((np.arange(C), -sizes))
    want_rank = np.empty(C, dtype=np.int64)
    want_rank[order] = np.arange(C)
    total = probe.comm_number_bytes(N)
    ws = torch.full((total,), 0x5A, dtype=torch.uint8, device=DEV)
    d_cnt, d_lab = _dev(sizes.astype(np.int32)), _dev(lab.astype(np.int32))
    rank, out = _padded(C, CANARY, torch.int32), _padded(N, CANARY, torch.int32)
    torch.cuda.synchronize()
    rc, offs = probe.comm_number(ctx, _ptr(ws), C, N, _ptr(d_cnt), _ptr(d_lab), _ptr(rank), _ptr(out))
    assert rc == OK and probe.sync(ctx) == OK
    assert np.array_equal(rank[:C].cpu().numpy(), want_rank), case
    assert np.array_equal(out[:N].cpu().numpy(), want_rank[lab]), case
    assert bool((rank[C:] == CANARY).all()) and bool((out[N:] == CANARY).all())
    assert np.array_equal(d_cnt.cpu().numpy(), sizes) and np.array_equal(d_lab.cpu().numpy(), lab)      # the inputs are left alone
    used = torch.zeros(total, dtype=torch.bool, device=DEV)
    for off, size in zip(offs, (8 * N, 8 * N, 4 * N, 4 * N, 8 * probe.hist_len(N, _bit_width(N)))):
        assert off % 256 == 0 and off + size <= total
        used[off:off + size] = True
    assert bool((ws[~used] == 0x5A).all()), case


def _insert(probe, ctx, c, w):
    """c, w: (rounds, 64) communities (negative: the lane sits out) and weights -> slot, own (rounds, 64; -7 where the lane sat
    out), and the table's 256 keys and sums; the 64 guard entries behind the table must be untouched."""
    rounds = c.shape[0]
    d_c, d_w = _dev(c.astype(np.int32).reshape(-1)), _dev(w.astype(np.uint64).view(np.int64).reshape(-1))
    slot, own = (torch.full((rounds * 64 + 16,), -7, dtype=torch.int32, device=DEV) for _ in range(2))
    key, val = _padded(320, CANARY, torch.int32), _padded(320, CANARY, torch.int64)
    torch.cuda.synchronize()
    assert probe.comm_insert(ctx, rounds, _ptr(d_c), _ptr(d_w), _ptr(slot), _ptr(own), _ptr(key), _ptr(val)) == OK and probe.sync(ctx) == OK
    assert bool((slot[rounds * 64:] == -7).all()) and bool((own[rounds * 64:] == -7).all())
    assert bool((key[256:320] == 0x5A5A5A5A).all()) and bool((val[256:320] == 0x5A5A5A5A5A5A5A5A).all())      # the guard behind the table
    assert bool((key[320:] == CANARY).all()) and bool((val[320:] == CANARY).all())
    return (slot[:rounds * 64].cpu().numpy().reshape(rounds, 64), own[:rounds * 64].cpu().numpy().reshape(rounds, 64), key[:256].cpu().numpy(),
            val[:256].cpu().numpy().view(np.uint64))


def _check_table(c, w, slot, own, key, val, full=()):
    """Every insert that found room: its slot holds its community, one owner per community, the slot's sum is the total of
    the lanes that brought it; the slots nobody claimed are empty."""
    refused = np.isin(c, np.array(full, dtype=np.int64))
    there = (c >= 0) & ~refused
    assert (slot[there] >= 0).all() and (slot[there] < 256).all() and (slot[refused] == -1).all() and (own[refused] == 0).all()
    assert np.array_equal(key[slot[there]], c[there])
    for comm in np.unique(c[there]):
        m = there & (c == comm)
        assert len(np.unique(slot[m])) == 1 and own[m].sum() == 1
        assert val[slot[m][0]] == np.add.reduce(w[m], dtype=np.uint64)
    free = np.setdiff1d(np.arange(256), slot[there])
    assert (key[free] == -1).all() and (val[free] == 0).all()


def test_table_insert_of_one_wave(probe, ctx):
    rng = np.random.default_rng(3)
    # 64 distinct communities: every lane owns its slot, the sums are the weights themselves (beyond 2^53: exact integers)
    c = rng.choice(2 ** 31 - 1, 64, replace=False).reshape(1, 64)
    w = rng.integers(1, 2 ** 62, (1, 64), dtype=np.uint64)
    slot, own, key, val = _insert(probe, ctx, c, w)
    assert (own == 1).all() and len(np.unique(slot)) == 64
    _check_table(c, w, slot, own, key, val)
    # 64 lanes on 3 communities: one owner each, every sum the total of its lanes
    c3 = rng.choice(np.array([5, 261, 1_000_000_007]), 64).reshape(1, 64)
    assert len(np.unique(c3)) == 3
    w3 = rng.integers(1, 2 ** 56, (1, 64), dtype=np.uint64)
    slot, own, key, val = _insert(probe, ctx, c3, w3)
    assert own.sum() == 3
    _check_table(c3, w3, slot, own, key, val)
    # 257 distinct communities over five rounds (64, 64, 64, 64, 1): the table is full when the last one comes — it alone gets
    # -1, owns nothing, and nothing is written past the table
    c5 = np.full(320, -1, dtype=np.int64)
    c5[:257] = rng.choice(2 ** 31 - 1, 257, replace=False)
    w5 = rng.integers(1, 2 ** 40, 320, dtype=np.uint64)
    c5, w5 = c5.reshape(5, 64), w5.reshape(5, 64)
    slot, own, key, val = _insert(probe, ctx, c5, w5)
    assert (slot[c5 >= 0] == -1).sum() == 1 and slot[4, 0] == -1 and (slot[c5 < 0] == -7).all()
    assert own[c5 >= 0].sum() == 256 and len(np.unique(slot[:4])) == 256
    _check_table(c5, w5, slot, own, key, val, full=(c5[4, 0],))
