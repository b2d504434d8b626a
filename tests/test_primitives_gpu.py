"""GPU: the library's shared primitives on their own, at the sizes where their branches switch.

  radix sort   gficf_radix_sort_kv (radix_sort.hip): 1..4 passes, uneven last pass, workgroups walking several tiles
               (M > 768 * 4096), stability, key bits above b ignored, nothing written past hist / okey / oval
  scan         gficf_exclusive_scan_i64 (ctx.hip): tile edges, the largest n the look-back workspace takes and one tile
               beyond, the 2^40 value limit, scans queued back to back, the epoch wrap at 2^22
  transpose    gficf_csc_transpose (transpose.hip): pairing (G <= 9000), plain with one gene range and with several
               (G > 36864), the cells-per-block floor of 16 and cap of 1024, long cells, empty cells and genes, explicit zeros

The sort and the scan are reached through tests/helpers/prim_probe.py; references are exact (NumPy / torch stable sorts and
integer cumulative sums)."""
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
