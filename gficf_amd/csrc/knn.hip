// knn.hip — exact k-nearest-neighbour search for gfx950 (MI355X): "next" row N2 of the hot path.
//
// Stands in for the caller's step in front of the Jaccard build,
//   neigh = uwot:::find_nn(data$pca$cells, k = k+1, include_self = T, method = "annoy", metric = dist.method)$idx
// (reference R/clustCells.R:57,60; uwot/Annoy are third-party and approximate).  This is an EXACT
// search: every query is compared with every point in f32 (Annoy stores f32 too) and the k
// smallest (distance, index) pairs are kept, ties broken by the smaller index — so the result is
// unique and checkable bit for bit against a CPU brute force.
//
// Metrics: manhattan (the reference's default, R/clustCells.R:46), euclidean, cosine (1 - cos), correlation (cosine of
// the mean-centred rows).
// Manhattan is |a-b| accumulation — VALU work, not a contraction, so no MFMA; euclidean and cosine
// share the same register-tiled kernel with a packed-fma chain in dimension order (an MFMA formulation
// |x|^2+|y|^2-2xy would change the rounding and with it the order of near-ties, and in f32 the matrix
// cores peak at the same 157 TFLOP/s as v_pk_fma_f32).
//
// Layout: points row-major f32 [N][dpad] (dpad = d rounded up to 4, zero padded; cosine: rows
// L2-normalised by the prepare kernel).  One workgroup = a tile of 64 queries x a slice of the
// candidates: the query tile stays in LDS ([dim][query]), candidate tiles of 128 points stream
// through a double-buffered LDS chunk of 16 dims; every thread accumulates a 4 x 8 block of
// distances in registers.  Per query a sorted list of the k best 64-bit keys
// (sortable(distance) << 32 | index) lives in LDS; a thread inserts a candidate only when it beats
// the list's last key (rare after the first tiles).  A query's row of the tile belongs to the 16 lanes
// of one wave, which take turns (wave-uniform loop, one elected lane per row and round): no locks.  A merge kernel
// writes the 1-based index matrix column-major — the layout the Jaccard ingest reads.
//
// Two forms of the same kernel, same bits:
//   plain  : every query tile against every candidate tile, the candidate range split S ways to fill the chip;
//   pruned : (default from 30 k points) the points are reordered so that a tile holds neighbours, every
//            (query tile, candidate tile) pair gets a triangle-inequality lower bound, and a query tile visits the
//            candidate tiles best bound first until the bound passes its queries' k-th best — see "pruned search:
//            preparation" in knn_prune.h.  When the bounds show no cluster structure, a device flag routes to the plain form.
//
// The tile kernel itself (k_knn_tiles, both forms) and its launchers are knn_tiles.h's: libgficf_transform.so's search of new
// cells is built from the same text.  The pruned search's preparation (its kernels, the pivot counts, its workspace) is
// knn_prune.h's.  Here: prepare, merge, split, checks, the run (KnnRun: one search, one function per step), entries.
#include <cfloat>
#include <cstdlib>
#include <vector>

#include "common.h"
#include "knn_prune.h"
#include "knn_tiles.h"

namespace {

__host__ __device__ inline int knn_dpad(int d) { return (d + 3) & ~3; }

// ----------------------------------------------------------------------------- prepare
// R matrix (column-major, f64 or f32) -> row-major f32 rows of dpad floats.  One thread per row;
// cosine: the row is divided by its f32 L2 norm (fma chain in dimension order), zero rows stay zero.
template <typename T>
__global__ __launch_bounds__(256) void k_knn_prepare(const T* __restrict__ X, int64_t n_rows, int d, int dpad, int64_t ld,
                                                     int metric, float* __restrict__ out, uint32_t* __restrict__ status) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rows) return;
  bool bad = false;
  float inv = 1.0f;
  bool scale = false;
  float mean = 0.0f;
  if (metric == GFICF_KNN_CORRELATION) {         // Pearson: centre the row first (f32 sum in dimension order / d)
    float sm = 0.0f;
    for (int t = 0; t < d; ++t) sm = sm + (float)X[(int64_t)t * ld + r];
    mean = sm / (float)d;
  }
  if (metric == GFICF_KNN_COSINE || metric == GFICF_KNN_CORRELATION) {
    float s = 0.0f;
    for (int t = 0; t < d; ++t) { const float v = (float)X[(int64_t)t * ld + r] - mean; s = fmaf(v, v, s); }
    const float nrm = sqrtf(s);
    scale = nrm > 0.0f;
    inv = nrm;
  }
  float* o = out + r * dpad;
  for (int t = 0; t < dpad; ++t) {
    float v = t < d ? (float)X[(int64_t)t * ld + r] : 0.0f;
    bad |= !(fabsf(v) <= FLT_MAX);              // NaN or +-Inf (also a double too large for f32)
    if (t < d) v = v - mean;
    if (scale) v = v / inv;
    o[t] = v;
  }
  if (bad) atomicOr(status, GFICF_ST_BAD_VALUE);
}

// ------------------------------------------------------------------------------ merge (the tile kernel: knn_tiles.h)
// k best of the S partial lists of a query (each ascending) -> 1-based ids / distances, column-major.
// perm_q (pruned search): the query's position in the caller's block.
__global__ __launch_bounds__(256) void k_knn_merge(const u64* __restrict__ part, int64_t n_q, int S, int kk, int metric,
                                                   const int32_t* __restrict__ perm_q, int32_t* __restrict__ idx,
                                                   float* __restrict__ dist, int64_t ld_out, const uint32_t* gate, uint32_t gate_want) {
  if (gate != nullptr && *gate != gate_want) return;
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= n_q) return;
  const int64_t oq = perm_q ? (int64_t)perm_q[q] : q;
  if (oq < 0) return;                                // padding row of the reordered query block
  int pos[KNN_MAX_SPLIT];
#pragma unroll
  for (int s = 0; s < KNN_MAX_SPLIT; ++s) pos[s] = 0;
  const u64* const base = part + q * S * kk;
  for (int t = 0; t < kk; ++t) {
    u64 best = ~0ull;
    int bs = 0;
#pragma unroll
    for (int s = 0; s < KNN_MAX_SPLIT; ++s) {
      if (s < S && pos[s] < kk) {
        const u64 v = base[s * kk + pos[s]];
        if (v < best) { best = v; bs = s; }
      }
    }
#pragma unroll
    for (int s = 0; s < KNN_MAX_SPLIT; ++s) pos[s] += (s == bs && best != ~0ull) ? 1 : 0;
    int32_t id = 0;
    float dv = INFINITY;
    if (best != ~0ull) {
      id = (int32_t)(uint32_t)best + 1;
      dv = sortable_f32((uint32_t)(best >> 32));
      if (metric == GFICF_KNN_EUCLIDEAN) dv = sqrtf(dv);
    }
    idx[(int64_t)t * ld_out + oq] = id;
    if (dist) dist[(int64_t)t * ld_out + oq] = dv;
  }
}

// ------------------------------------------------------------------------------ split, form, checks
int knn_split(const gficf_ctx* ctx, int64_t n_q, int64_t N) {
  const int64_t n_qt = gficf_ceil_div(n_q > 0 ? n_q : 1, KNN_TQ), n_ct = gficf_ceil_div(N > 0 ? N : 1, KNN_TC);
  // enough work items for ~8 per CU, but every candidate slice at least 8 tiles long
  int64_t S = gficf_ceil_div((int64_t)ctx->num_cus * 8, n_qt);
  if (S > n_ct / 8) S = n_ct / 8;
  if (S > KNN_MAX_SPLIT) S = KNN_MAX_SPLIT;
  if (S < 1) S = 1;
  if (const char* e = getenv("GFICF_KNN_SPLIT")) {   // tuning knob / test hook
    const int v = atoi(e);
    if (v >= 1 && v <= KNN_MAX_SPLIT) S = v;
  }
  return (int)S;
}

// The pruned search pays for its preparation (~1 ms at 100 k points) only on larger inputs; the bounds of a query
// tile have to fit LDS.  GFICF_KNN_PRUNE=0 / 1 forces it off / on (test hook): a search reads it once (knn_prune_env) and
// carries the value in its run.
constexpr int64_t KNN_PRUNE_MIN_N = 30000;
constexpr int64_t KNN_PRUNE_MAX_TILES = 8192;
constexpr int KNN_PRUNE_UNSET = -1;          // else 0 (forced off) or 1 (set and non-zero: forced on)
int knn_prune_env() {
  const char* e = getenv("GFICF_KNN_PRUNE");
  return !e ? KNN_PRUNE_UNSET : atoi(e) != 0 ? 1 : 0;
}
bool knn_use_prune(int64_t N, int prune_env) {
  const int64_t n_ct = gficf_ceil_div(N > 0 ? N : 1, KNN_TC);
  if (n_ct < 2 || n_ct > KNN_PRUNE_MAX_TILES) return false;
  if (prune_env != KNN_PRUNE_UNSET) return prune_env != 0;
  return N >= KNN_PRUNE_MIN_N;
}

int knn_check(int64_t N, int d, int k, int metric) {
  if (N < 0 || d < 0 || k < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "negative size");
  if (N > 0x7FFFFFFFll) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "N = %lld exceeds int32 ids", (long long)N);
  if (d > KNN_MAX_D) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "d = %d exceeds %d dimensions", d, KNN_MAX_D);
  if (k > GFICF_KNN_MAX_K) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "k = %d exceeds GFICF_KNN_MAX_K = %d", k, GFICF_KNN_MAX_K);
  if (k > N) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "k = %d neighbours asked of N = %lld points", k, (long long)N);
  if (!gficf_knn_metric_ok(metric)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "unknown metric %d", metric);
  return GFICF_OK;
}

inline dim3 knn_blocks(int64_t n) { return dim3((unsigned)gficf_ceil_div(n, 256)); }      // one thread per item, 256 a workgroup

// ------------------------------------------------------------------------------ the run
// One search of a query block on checked arguments (gficf_knn_search_device), or the first two steps of one
// (gficf_knn_pivot_order_device: N queries, k = 1, no outputs); the entries drive its steps.  Everything is enqueued on the
// context's stream, nothing synchronises.  The pruned form is
//   assign_pivots -> clear_padded_copies -> lay_out (candidates) -> lay_out (queries) -> bounds -> search_both_forms.
struct KnnRun {
  gficf_ctx* ctx;
  hipStream_t st;
  const float* X;                  // the points, [N][dpad]
  int64_t N;
  int d, dpad, nq4, metric, k;     // metric: the search's (gficf_knn_search_metric)
  int64_t q_begin, n_q;            // the query block: rows q_begin .. of X
  int32_t* idx;                    // the outputs, column-major with ld_out rows
  float* dist;
  int64_t ld_out;
  KnnPruneWs w;                    // carved from prune_ws; all zero when the run takes no pivots (prune_ws == nullptr)
  int prune_env;                   // GFICF_KNN_PRUNE as read for this call: KNN_PRUNE_UNSET, 0 or 1

  KnnRun(gficf_ctx* c, const float* points, int64_t n, int d_, int search_metric, int k_, int64_t qb, int64_t nq, int32_t* idx_, float* dist_,
         int64_t ld, void* prune_ws, int env)
      : ctx(c), st(c->stream), X(points), N(n), d(d_), dpad(knn_dpad(d_)), nq4(knn_dpad(d_) >> 2), metric(search_metric), k(k_), q_begin(qb),
        n_q(nq), idx(idx_), dist(dist_), ld_out(ld), w(prune_ws ? knn_prune_ws((char*)prune_ws, nq, n, knn_dpad(d_), k_) : KnnPruneWs{}),
        prune_env(env) {}

  // The plain form and its merge: every query tile against every candidate tile, the candidate range split S ways.  Ungated
  // (gate == nullptr) when the data set does not prune; otherwise both run only if *gate == gate_want.
  int search_plain(u64* part, const uint32_t* gate, uint32_t gate_want) {
    KnnTileArgs a = knn_plain_args(X + q_begin * dpad, n_q, X, N, d, dpad, k, knn_split(ctx, n_q, N), part);
    a.gate = gate; a.gate_want = gate_want;
    const int rc = knn_launch_m<false>(ctx, metric, a);
    if (rc) return rc;
    hipLaunchKernelGGL(k_knn_merge, knn_blocks(n_q), dim3(256), 0, st, part, n_q, a.S, k, metric, (const int32_t*)nullptr, idx, dist, ld_out, gate, gate_want);
    GFICF_HIP_CHECK(hipGetLastError());
    return GFICF_OK;
  }

  // out[q] = the nearest (1-based) of the np rows of P to row q of Q: the tile kernel at k = 1 and its merge.  w.apart
  // serves both assignments.
  int nearest(const float* Q, int64_t nq, const float* P, int64_t np, int32_t* out) {
    const int rc = knn_launch_m<false>(ctx, metric, knn_plain_args(Q, nq, P, np, d, dpad, 1, 1, w.apart));
    if (rc) return rc;
    hipLaunchKernelGGL(k_knn_merge, knn_blocks(nq), dim3(256), 0, st, w.apart, nq, 1, 1, metric, (const int32_t*)nullptr, out, (float*)nullptr, nq, (const uint32_t*)nullptr, 0u);
    return GFICF_OK;
  }

  // pivots = C evenly spaced points, every point's nearest pivot; coarse pivots = every (C / Cc)-th fine pivot, every fine
  // pivot's nearest coarse one
  int assign_pivots() {
    const int64_t C = w.C, Cc = knn_coarse(C);
    hipLaunchKernelGGL(k_knn_gather_rows, knn_blocks(C * nq4), dim3(256), 0, st, X, (const int32_t*)nullptr, C, nq4, N / C, w.pivots);
    int rc = nearest(X, N, w.pivots, C, w.pivot_of);
    if (rc) return rc;
    hipLaunchKernelGGL(k_knn_gather_rows, knn_blocks(Cc * nq4), dim3(256), 0, st, w.pivots, (const int32_t*)nullptr, Cc, nq4, C / Cc, w.coarse);
    rc = nearest(w.pivots, C, w.coarse, Cc, w.coarse_of);
    if (rc) return rc;
    GFICF_HIP_CHECK(hipGetLastError());
    return GFICF_OK;
  }

  // order_out = the n points from `first` on, sorted by (coarse, fine) pivot; stable: ties keep index order.  Their keys
  // are left in w.key_tmp.
  int sort_cells(int64_t first, int64_t n, int32_t* order_out) {
    hipLaunchKernelGGL(k_knn_sort_elems, knn_blocks(n), dim3(256), 0, st, w.pivot_of + first, w.coarse_of, n, w.kv0);
    GFICF_HIP_CHECK(hipGetLastError());
    return gficf_radix_sort_kv(ctx, w.kv0, w.kv1, w.hist, n, KNN_CELL_KEY_BITS, (uint32_t*)w.key_tmp, (uint32_t*)order_out);
  }

  // the padded copies of candidates and queries: zero rows, ids -1, until lay_out fills in the real ones
  int clear_padded_copies() {
    GFICF_HIP_CHECK(hipMemsetAsync(w.xp, 0, sizeof(float) * (size_t)w.xrows * dpad, st));
    GFICF_HIP_CHECK(hipMemsetAsync(w.qp, 0, sizeof(float) * (size_t)w.qrows * dpad, st));
    GFICF_HIP_CHECK(hipMemsetAsync(w.perm_x, 0xFF, sizeof(int32_t) * (size_t)w.xrows, st));
    GFICF_HIP_CHECK(hipMemsetAsync(w.perm_q, 0xFF, sizeof(int32_t) * (size_t)w.qrows, st));
    return GFICF_OK;
  }

  // The n points from `first` on (rows of src) sorted by cell and laid out cell by cell into dst, every cell starting on a
  // boundary of the tile size T; perm_pad = the id of every padded row (relative to first), tile_n = the real rows of every
  // tile.  Both calls use w.key_tmp, w.rank, w.kv0, w.kv1 and w.hist, one after the other.
  int lay_out(int64_t first, int64_t n, int T, const float* src, float* dst, int32_t* perm_pad, int64_t n_tiles, int32_t* tile_n) {
    int rc = sort_cells(first, n, w.perm_sorted);
    if (rc) return rc;
    hipLaunchKernelGGL(k_knn_cell_heads, knn_blocks(n + 1), dim3(256), 0, st, w.key_tmp, n, w.rank);
    rc = gficf_exclusive_scan_i64(ctx, w.rank, n + 1);
    if (rc) return rc;
    hipLaunchKernelGGL(k_knn_cell_starts, knn_blocks(n + 1), dim3(256), 0, st, w.key_tmp, w.rank, n, w.cstart);
    hipLaunchKernelGGL(k_knn_cell_offsets, dim3(1), dim3(1024), 0, st, w.cstart, w.rank + n, T, w.pstart);
    hipLaunchKernelGGL(k_knn_pad_scatter, knn_blocks(n * nq4), dim3(256), 0, st, w.key_tmp, w.rank, w.cstart, w.pstart, w.perm_sorted, n, nq4,
                       src, dst, perm_pad);
    hipLaunchKernelGGL(k_knn_tile_counts, knn_blocks(n_tiles), dim3(256), 0, st, perm_pad, n_tiles, T, tile_n);
    GFICF_HIP_CHECK(hipGetLastError());
    return GFICF_OK;
  }

  // centre and radius of every candidate tile; bound of every (query tile, candidate tile) pair, and the count of the pairs
  // that are certain to be pruned
  template <int METRIC>
  void bounds_m() {
    hipLaunchKernelGGL(k_knn_tile_stats<METRIC>, dim3((unsigned)w.n_ct), dim3(KNN_TC), 0, st, w.xp, w.tile_n, d, dpad, w.centers, w.radius);
    hipLaunchKernelGGL(k_knn_lb<METRIC>, dim3((unsigned)w.n_qt), dim3(256), (size_t)KNN_TQ * dpad * sizeof(float), st, w.qp, w.qtile_n, d, dpad, w.centers,
                       w.radius, w.tile_n, k, w.n_ct, w.lb, w.counters);
  }
  int bounds() {
    GFICF_HIP_CHECK(hipMemsetAsync(w.counters, 0, 32, st));
    switch (metric) {
      case GFICF_KNN_MANHATTAN: bounds_m<GFICF_KNN_MANHATTAN>(); break;
      case GFICF_KNN_EUCLIDEAN: bounds_m<GFICF_KNN_EUCLIDEAN>(); break;
      default: bounds_m<GFICF_KNN_COSINE>(); break;
    }
    GFICF_HIP_CHECK(hipGetLastError());
    return GFICF_OK;
  }

  // The form is chosen on the device (k_knn_choose: the plain one when the bounds say there is nothing to prune, unless
  // GFICF_KNN_PRUNE forces the pruned one); both are enqueued and the one not chosen returns at once.  Plain: as ever, on
  // the caller's rows.  Pruned: over the reordered copies, tiles in best-first order with early exit, and back to the
  // caller's order through perm_q.
  int search_both_forms() {
    uint32_t* const flag = (uint32_t*)(w.counters + 2);
    hipLaunchKernelGGL(k_knn_choose, dim3(1), dim3(1), 0, st, w.counters, (uint32_t)(prune_env == 1), flag);
    int rc = search_plain(w.part_plain, flag, 1u);
    if (rc) return rc;
    KnnTileArgs a = knn_plain_args(w.qp, w.qrows, w.xp, w.xrows, d, dpad, k, 1, w.part);
    a.perm_x = w.perm_x; a.lb = w.lb; a.tile_n = w.tile_n; a.qtile_n = w.qtile_n;
    a.gate = flag; a.gate_want = 0u;
    rc = knn_launch_m<true>(ctx, metric, a);
    if (rc) return rc;
    hipLaunchKernelGGL(k_knn_merge, knn_blocks(w.qrows), dim3(256), 0, st, w.part, w.qrows, 1, k, metric, (const int32_t*)w.perm_q, idx, dist, ld_out, (const uint32_t*)flag, 0u);
    GFICF_HIP_CHECK(hipGetLastError());
    return GFICF_OK;
  }
};

}  // namespace

extern "C" {

int gficf_knn_dpad(int d) { return (d < 0 || d > KNN_MAX_D) ? -1 : knn_dpad(d); }

int gficf_knn_prepare_device(gficf_ctx* ctx, const void* d_X, int x_is_f64, int64_t n_rows, int d, int64_t ld, int metric,
                             float* d_point_rows) {
  GFICF_CTX_ENTER(ctx);
  int rc = knn_check(n_rows, d, 0, metric);
  if (rc) return rc;
  if (n_rows == 0 || d == 0) return GFICF_OK;
  if (!d_X || !d_point_rows) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  if (ld < n_rows) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "ld = %lld < n_rows = %lld", (long long)ld, (long long)n_rows);
  const unsigned blocks = (unsigned)gficf_ceil_div(n_rows, 256);
  if (x_is_f64)
    hipLaunchKernelGGL(k_knn_prepare<double>, dim3(blocks), dim3(256), 0, ctx->stream, (const double*)d_X, n_rows, d, knn_dpad(d), ld, metric, d_point_rows, ctx->d_status);
  else
    hipLaunchKernelGGL(k_knn_prepare<float>, dim3(blocks), dim3(256), 0, ctx->stream, (const float*)d_X, n_rows, d, knn_dpad(d), ld, metric, d_point_rows, ctx->d_status);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

size_t gficf_knn_workspace_bytes(gficf_ctx* ctx, int64_t n_queries, int64_t N, int k) {
  if (!ctx || n_queries <= 0 || N <= 0 || k <= 0) return 256;
  // the larger of the plain form's partial lists at the current split and — where the tile count admits pivots — the pruned
  // form's carve at the widest rows, whose own plain lists are sized for KNN_MAX_SPLIT
  const size_t small = (size_t)n_queries * (size_t)knn_split(ctx, n_queries, N) * (size_t)k * sizeof(u64) + 256;
  const size_t pruned = gficf_ceil_div(N, KNN_TC) <= KNN_PRUNE_MAX_TILES ? knn_prune_ws(nullptr, n_queries, N, knn_dpad(KNN_MAX_D), k).total : 0;
  return small > pruned ? small : pruned;
}

int gficf_knn_search_device(gficf_ctx* ctx, const float* d_points, int64_t N, int d, int k, int metric, int64_t q_begin,
                            int64_t q_end, void* d_ws, size_t ws_bytes, int32_t* d_idx, float* d_dist, int64_t ld_out) {
  GFICF_CTX_ENTER(ctx);
  int rc = knn_check(N, d, k, metric);
  if (rc) return rc;
  if (q_begin < 0 || q_end < q_begin || q_end > N)
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "query range [%lld, %lld) outside [0, %lld]", (long long)q_begin, (long long)q_end, (long long)N);
  const int64_t n_q = q_end - q_begin;
  if (n_q == 0 || k == 0) return GFICF_OK;
  if (d == 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "points have no dimensions");
  if (!d_points || !d_ws || !d_idx) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  if (ld_out < n_q) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "ld_out = %lld < number of queries %lld", (long long)ld_out, (long long)n_q);
  if (ws_bytes < gficf_knn_workspace_bytes(ctx, n_q, N, k)) GFICF_FAIL(GFICF_ERR_CAPACITY, "kNN workspace too small");
  const int prune_env = knn_prune_env();
  const bool prune = knn_use_prune(N, prune_env);
  KnnRun r(ctx, d_points, N, d, gficf_knn_search_metric(metric), k, q_begin, n_q, d_idx, d_dist, ld_out, prune ? d_ws : nullptr, prune_env);
  if (!prune) return r.search_plain((u64*)d_ws, nullptr, 0u);
  const KnnPruneWs& w = r.w;
  rc = r.assign_pivots();
  if (!rc) rc = r.clear_padded_copies();
  if (!rc) rc = r.lay_out(0, N, KNN_TC, d_points, w.xp, w.perm_x, w.n_ct, w.tile_n);
  if (!rc) rc = r.lay_out(q_begin, n_q, KNN_TQ, d_points + q_begin * r.dpad, w.qp, w.perm_q, w.n_qt, w.qtile_n);
  if (!rc) rc = r.bounds();
  if (!rc) rc = r.search_both_forms();
  return rc;
}

/* The cell order of the pruned search, for callers that want ids with LOCALITY (the sharded Jaccard build's halo form,
 * gficf_amd/dist.py): d_order[p] = 0-based row of the point at position p when the points are sorted by their (coarse, fine)
 * pivot — KnnRun's assign_pivots and sort_cells, the very steps the pruned search starts with, nothing else.  Points whose
 * nearest neighbours share their pivot cell end up next to each other, so a contiguous block of the order names few rows
 * outside itself.  A function of the points alone: every rank of a sharded job computes the same order from the same
 * (all-gathered) points.  Workspace as for a search with N queries.  Pivots whenever the tile count admits them, down to two
 * for N <= 128; GFICF_KNN_PRUNE has no say here. */
int gficf_knn_pivot_order_device(gficf_ctx* ctx, const float* d_points, int64_t N, int d, int metric, void* d_ws, size_t ws_bytes,
                                 int32_t* d_order) {
  GFICF_CTX_ENTER(ctx);
  int rc = knn_check(N, d, 1, metric);
  if (rc) return rc;
  if (N == 0) return GFICF_OK;
  if (d == 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "points have no dimensions");
  if (!d_points || !d_ws || !d_order) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  if (ws_bytes < gficf_knn_workspace_bytes(ctx, N, N, 1)) GFICF_FAIL(GFICF_ERR_CAPACITY, "kNN workspace too small");
  if (gficf_ceil_div(N, KNN_TC) > KNN_PRUNE_MAX_TILES) {      // no pivots at this size: the order as given
    hipLaunchKernelGGL(k_knn_iota, knn_blocks(N), dim3(256), 0, ctx->stream, d_order, N);
    GFICF_HIP_CHECK(hipGetLastError());
    return GFICF_OK;
  }
  KnnRun r(ctx, d_points, N, d, gficf_knn_search_metric(metric), 1, 0, N, nullptr, nullptr, N, d_ws, KNN_PRUNE_UNSET);
  rc = r.assign_pivots();
  if (!rc) rc = r.sort_cells(0, N, d_order);
  return rc;
}

int gficf_knn_host(gficf_ctx* ctx, const double* X, int64_t N, int d, int64_t ld, int k, int metric, int32_t* idx, double* dist) {
  GFICF_CTX_ENTER(ctx);
  int rc = knn_check(N, d, k, metric);
  if (rc) return rc;
  if (N == 0 || k == 0) return GFICF_OK;
  if (d == 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "points have no dimensions");
  if (!X || !idx) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL host pointer");
  if (ld < N) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "ld = %lld < N = %lld", (long long)ld, (long long)N);
  const size_t xb = sizeof(double) * (size_t)ld * (size_t)d, pb = sizeof(float) * (size_t)N * (size_t)knn_dpad(d);
  const size_t wsb = gficf_knn_workspace_bytes(ctx, N, N, k), ob = (size_t)N * (size_t)k;
  void *d_X = nullptr, *d_P = nullptr, *d_ws = nullptr, *d_out = nullptr;
  gficf_host_io io{ctx, "gficf_knn_host"};
  io.get(GFICF_SLOT_STAGE0, xb, &d_X);
  io.get(GFICF_SLOT_STAGE1, pb, &d_P);
  io.get(GFICF_SLOT_STAGE2, wsb, &d_ws);
  io.get(GFICF_SLOT_DEV_SIG_ORDER, ob * (sizeof(int32_t) + sizeof(float)), &d_out);
  io.up(d_X, X, xb);
  std::vector<float> hd;
  if (io.ok()) {
    int32_t* d_idx = (int32_t*)d_out;
    float* d_dist = (float*)(d_idx + ob);
    rc = gficf_knn_prepare_device(ctx, d_X, 1, N, d, ld, metric, (float*)d_P);
    if (!rc) rc = gficf_knn_search_device(ctx, (const float*)d_P, N, d, k, metric, 0, N, d_ws, wsb, d_idx, dist ? d_dist : nullptr, N);
    gficf_advise_hugepages(idx, ob * sizeof(int32_t));             // (fresh R matrices: first touched by the copies below)
    if (dist) gficf_advise_hugepages(dist, ob * sizeof(double));
    if (!rc) io.down(idx, d_idx, ob * sizeof(int32_t));
    if (!rc && io.ok() && dist) {
      hd.resize(ob);
      io.down(hd.data(), d_dist, ob * sizeof(float));
    }
  }
  rc = io.finish(rc);
  if (rc) return rc;
  if (dist)
    for (size_t t = 0; t < ob; ++t) dist[t] = (double)hd[t];
  return GFICF_OK;
}

}  // extern "C"
