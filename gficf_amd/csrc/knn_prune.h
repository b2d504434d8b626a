// knn_prune.h — the preparation of knn.hip's pruned search: the pivot and cell-layout kernels, the per-tile bounds, the choice
// between the two forms, the pivot counts and the workspace they are carved from.  Only knn.hip includes it (the tile kernel both
// forms run is knn_tiles.h's; the driver that enqueues all this, KnnRun, is knn.hip's).
#pragma once

#include <cstdlib>

#include "common.h"
#include "knn_tiles.h"

namespace {

// the search's limits: knn.hip checks them; the bound kernels' LDS and the workspace below are sized by them
constexpr int KNN_MAX_D = 128;
constexpr int KNN_MAX_SPLIT = 16;

// ------------------------------------------------------------------ pruned search: preparation
// The exact search skips whole candidate tiles that provably cannot contribute: with a centre c_t and radius r_t
// per candidate tile (r_t = largest distance of a tile point to c_t), every point x of the tile is at least
//   min over the query tile's points q of dist(q, c_t)  -  r_t
// away from every query of the tile (triangle inequality: manhattan and euclidean directly; cosine through the
// euclidean distance e of the unit vectors, 1 - cos = e^2 / 2).  For the bound to bite, the points are reordered so
// that a tile holds neighbours: every point is assigned to its nearest of ~N/128 pivots (the tile kernel itself
// with the pivots as candidates and k = 1) and the points are sorted by pivot.
constexpr float KNN_LB_SLACK = 1e-4f;      // relative slack on the bound: f32 rounding of 128-dim sums is ~1e-5

__global__ __launch_bounds__(256) void k_knn_gather_rows(const float* __restrict__ src, const int32_t* __restrict__ rows, int64_t n,
                                                         int nq4, int64_t stride_or_zero, float* __restrict__ dst) {
  // dst row r = src row rows[r] (rows == nullptr: src row r * stride_or_zero — evenly spaced pivots)
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n * nq4) return;
  const int64_t r = e / nq4;
  const int q4 = (int)(e % nq4);
  const int64_t sr = rows ? (int64_t)rows[r] : r * stride_or_zero;
  reinterpret_cast<float4*>(dst)[e] = reinterpret_cast<const float4*>(src)[sr * nq4 + q4];
}

__global__ __launch_bounds__(256) void k_knn_iota(int32_t* __restrict__ v, int64_t n) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n) v[e] = (int32_t)e;
}

// sort element of point e: key << 32 | e, key = (coarse pivot of its fine pivot - 1) << 12 | (fine pivot - 1)   (ids 1-based, at most
// 4096 fine and 256 coarse pivots: 20 bits, two passes of the sort; stable, so the points of one cell keep the order of e)
constexpr int KNN_CELL_KEY_BITS = 20;
__global__ __launch_bounds__(256) void k_knn_sort_elems(const int32_t* __restrict__ pivot_of, const int32_t* __restrict__ coarse_of,
                                                        int64_t n, u64* __restrict__ kv) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n) {
    const int32_t f = pivot_of[e];
    kv[e] = ((u64)(uint32_t)(((coarse_of[f - 1] - 1) << 12) | (f - 1)) << 32) | (u64)e;
  }
}

// distance used by the bounds: the metric itself for manhattan, the euclidean distance otherwise
template <int METRIC>
__device__ inline float knn_bound_dist(const float* __restrict__ a, const float* __restrict__ b, int d) {
  float acc = 0.0f;
  for (int t = 0; t < d; ++t) {
    const float df = a[t] - b[t];
    acc = METRIC == GFICF_KNN_MANHATTAN ? acc + fabsf(df) : fmaf(df, df, acc);
  }
  return METRIC == GFICF_KNN_MANHATTAN ? acc : sqrtf(acc);
}

// one workgroup of 128 threads per candidate tile: centre = mean of the tile's points, radius = largest distance to it
template <int METRIC>
__global__ __launch_bounds__(KNN_TC) void k_knn_tile_stats(const float* __restrict__ X, const int32_t* __restrict__ tile_n, int d, int dpad,
                                                           float* __restrict__ centers, float* __restrict__ radius) {
  __shared__ float s_c[KNN_MAX_D];
  __shared__ float s_r[KNN_TC / 64];
  const int64_t t = blockIdx.x, j0 = t * KNN_TC;
  const int n = tile_n[t];
  if (n <= 0) { if (threadIdx.x == 0) radius[t] = -1.0f; return; }      // padding tile: marked empty
  for (int dim = threadIdx.x; dim < dpad; dim += KNN_TC) {
    float sum = 0.0f;
    for (int p = 0; p < n; ++p) sum += X[(j0 + p) * dpad + dim];
    const float c = sum / (float)n;
    s_c[dim] = c;
    centers[(int64_t)dim * gridDim.x + t] = c;        // [dim][tile]: k_knn_lb reads a dim of consecutive tiles at a time
  }
  __syncthreads();
  float r = 0.0f;
  if ((int)threadIdx.x < n) r = knn_bound_dist<METRIC>(X + (j0 + threadIdx.x) * dpad, s_c, d);
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) r = fmaxf(r, __shfl_xor(r, w));
  if ((threadIdx.x & 63) == 0) s_r[threadIdx.x >> 6] = r;
  __syncthreads();
  if (threadIdx.x == 0) radius[t] = fmaxf(s_r[0], s_r[1]);
}

// one workgroup per query tile: lb[qt][ct] = the bound above, in the domain of the keys (manhattan: distance,
// euclidean: squared distance, cosine: 1 - cos), lowered by the slack; never negative.
// It also counts the pairs that are certain to be pruned, for the choice between the two forms of the search: any
// candidate tile with at least kk points bounds every query's k-th best from above by max_q dist(q, centre) + radius
// (all its points are that close); U = the smallest such bound over the tiles; a pair with lb > U is never visited.
template <int METRIC>
__global__ __launch_bounds__(256) void k_knn_lb(const float* __restrict__ Q, const int32_t* __restrict__ qtile_n, int d, int dpad,
                                                const float* __restrict__ centers, const float* __restrict__ radius,
                                                const int32_t* __restrict__ tile_n, int kk, int64_t n_ct, float* __restrict__ lb,
                                                unsigned long long* __restrict__ counters) {
  extern __shared__ __attribute__((aligned(16))) float s_q[];   // [dpad][KNN_TQ]: a dimension of the 64 queries is contiguous (rows beyond nq: zeros, never used)
  __shared__ float s_u[4];
  const int64_t qt = blockIdx.x, q0 = qt * KNN_TQ;
  const int nq = qtile_n[qt];
  if (nq <= 0) return;                               // padding tile: its workgroup of the search exits at once
  for (int e = threadIdx.x; e < KNN_TQ * dpad; e += 256) {
    const int row = e / dpad, dim = e % dpad;
    s_q[dim * KNN_TQ + row] = row < nq ? Q[(q0 + row) * dpad + dim] : 0.0f;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // cosine / correlation keys are 1 - dot of unit vectors, a d-term f32 sum: its computed value is within d * 2^-24 of the
  // exact one (sum |a_i b_i| <= 1), plus a few roundings of the normalisation; the absolute slack is twice that bound
  const float key_abs_slack = (float)(d + 8) * 1.1920929e-7f;
  auto to_key = [key_abs_slack](float e, float slack_sign) {     // distance of the bound's metric -> key domain, pushed by the slack
    if (METRIC == GFICF_KNN_MANHATTAN) return e;
    if (METRIC == GFICF_KNN_EUCLIDEAN) return e * e * (1.0f + slack_sign * KNN_LB_SLACK);
    return 0.5f * e * e * (1.0f + slack_sign * KNN_LB_SLACK) + slack_sign * key_abs_slack;
  };
  // one thread per candidate tile: the distance of EVERY query of the tile to the candidate tile's centre c (round 6; through round 5
  // the bound went through the query tile's own centre, dist(cq, c) - rq - r: in 50 dimensions the queries all sit at nearly the same
  // distance from c, far above that — on the config-3 stand-in 97 % of the pairs are provably out of reach this way, 82 % before).
  // (Screening the pairs with the old bound first and refining only those it leaves in reach was tried: its own upper bound of the k-th
  // best is so loose in 50 dimensions that every pair is left in reach — slower by the screening.)
  // Every point x of the candidate tile is within r of c, so  dist(q, x) >= min_q dist(q, c) - r  and  <= max_q dist(q, c) + r.
  float u = INFINITY;                                // upper bound of the queries' k-th best (key domain)
  for (int64_t c = threadIdx.x; c < n_ct; c += 256) {
    const float r = radius[c];
    if (r < 0.0f) { lb[qt * n_ct + c] = INFINITY; continue; }      // empty candidate tile: never visited
    float mn = INFINITY, mx = 0.0f;
    for (int g0 = 0; g0 < nq; g0 += 16) {             // sixteen queries at a time (their coordinates: LDS broadcast reads)
      float acc[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[j] = 0.0f;
      for (int t = 0; t < d; ++t) {
        const float cv = centers[(int64_t)t * n_ct + c];            // [dim][tile]: consecutive threads, consecutive tiles
        const float4* q4 = reinterpret_cast<const float4*>(s_q + t * KNN_TQ + g0);     // four 16 B broadcast reads
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4) {
          const float4 q = q4[j4];
          const float qa[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float df = qa[j] - cv;
            acc[4 * j4 + j] = METRIC == GFICF_KNN_MANHATTAN ? acc[4 * j4 + j] + fabsf(df) : fmaf(df, df, acc[4 * j4 + j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if (g0 + j < nq) {
          const float e = METRIC == GFICF_KNN_MANHATTAN ? acc[j] : sqrtf(acc[j]);
          mn = fminf(mn, e); mx = fmaxf(mx, e);
        }
      }
    }
    float b = mn - r - KNN_LB_SLACK * (mn + r);
    b = b > 0.0f ? to_key(b, -1.0f) : 0.0f;
    lb[qt * n_ct + c] = b > 0.0f ? b : 0.0f;
    if (tile_n[c] >= kk) u = fminf(u, to_key((mx + r) * (1.0f + KNN_LB_SLACK), 1.0f));
  }
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) u = fminf(u, __shfl_xor(u, w));
  if (lane == 0) s_u[wave] = u;
  __syncthreads();
  const float U = fminf(fminf(s_u[0], s_u[1]), fminf(s_u[2], s_u[3]));
  int npr = 0, np = 0;                               // pairs certain to be pruned / all pairs with a real candidate tile
  for (int64_t c = threadIdx.x; c < n_ct; c += 256) {
    const float b = lb[qt * n_ct + c];               // this thread's own stores
    if (b < INFINITY) { ++np; npr += b > U ? 1 : 0; }
  }
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) { npr += __shfl_xor(npr, w); np += __shfl_xor(np, w); }
  if (lane == 0) { atomicAdd(counters, (unsigned long long)npr); atomicAdd(counters + 1, (unsigned long long)np); }
}

// flag = 1 (plain search) when fewer than half of the (query tile, candidate tile) pairs are certain to be pruned: the
// data has too little cluster structure, and the plain form with its split candidate range runs faster
__global__ void k_knn_choose(const unsigned long long* __restrict__ counters, uint32_t force, uint32_t* __restrict__ flag) {
  *flag = force ? 0u : (2ull * counters[0] < counters[1] ? 1u : 0u);
}

// ---- cells padded to whole tiles
// The points are sorted by cell key; every cell is moved to a position that is a multiple of the tile size T, so that
// no tile holds points of two cells (a straddling tile spans both and its radius makes it unprunable for everybody
// near either cell).  Rows in between are padding: zero coordinates, id -1, never a candidate, never a query.
__global__ __launch_bounds__(256) void k_knn_cell_heads(const int32_t* __restrict__ keys, int64_t n, int64_t* __restrict__ flags) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p > n) return;
  flags[p] = (p < n && (p == 0 || keys[p] != keys[p - 1])) ? 1 : 0;
}
// rank[] = exclusive scan of the head flags (rank[n] = number of cells); cstart[c] = first sorted position of cell c
__global__ __launch_bounds__(256) void k_knn_cell_starts(const int32_t* __restrict__ keys, const int64_t* __restrict__ rank, int64_t n,
                                                         int32_t* __restrict__ cstart) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p > n) return;
  if (p == n) { cstart[rank[n]] = (int32_t)n; return; }
  if (p == 0 || keys[p] != keys[p - 1]) cstart[rank[p]] = (int32_t)p;
}
// one workgroup: pstart[c] = padded start of cell c (exclusive scan of the cells' sizes rounded up to T), pstart[n_cells] =
// padded total; at most 4097 cells
__global__ __launch_bounds__(1024) void k_knn_cell_offsets(const int32_t* __restrict__ cstart, const int64_t* __restrict__ n_cells_p, int T,
                                                           int32_t* __restrict__ pstart) {
  __shared__ int s_part[1024];
  __shared__ int s_total;
  const int n_cells = (int)*n_cells_p;
  const int per = (n_cells + 1023) / 1024;
  const int c0 = threadIdx.x * per;
  int sum = 0;
  for (int c = c0; c < c0 + per && c < n_cells; ++c) sum += (cstart[c + 1] - cstart[c] + T - 1) / T * T;
  s_part[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int t = 0; t < 1024; ++t) { const int v = s_part[t]; s_part[t] = run; run += v; }
    s_total = run;
  }
  __syncthreads();
  int run = s_part[threadIdx.x];
  for (int c = c0; c < c0 + per && c < n_cells; ++c) { pstart[c] = run; run += (cstart[c + 1] - cstart[c] + T - 1) / T * T; }
  if (threadIdx.x == 0) pstart[n_cells] = s_total;
}
// padded position of every sorted point; copy of its row; its id
__global__ __launch_bounds__(256) void k_knn_pad_scatter(const int32_t* __restrict__ keys, const int64_t* __restrict__ rank,
                                                         const int32_t* __restrict__ cstart, const int32_t* __restrict__ pstart,
                                                         const int32_t* __restrict__ perm, int64_t n, int nq4,
                                                         const float* __restrict__ src, float* __restrict__ dst, int32_t* __restrict__ perm_pad) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n * nq4) return;
  const int64_t p = e / nq4;
  const int q4 = (int)(e % nq4);
  const bool head = p == 0 || keys[p] != keys[p - 1];
  const int64_t c = rank[p] + (head ? 1 : 0) - 1;
  const int64_t pp = (int64_t)pstart[c] + (p - cstart[c]);
  const int32_t id = perm[p];
  reinterpret_cast<float4*>(dst)[pp * nq4 + q4] = reinterpret_cast<const float4*>(src)[(int64_t)id * nq4 + q4];
  if (q4 == 0) perm_pad[pp] = id;
}
// real rows per tile (they are a prefix of the tile)
__global__ __launch_bounds__(256) void k_knn_tile_counts(const int32_t* __restrict__ perm_pad, int64_t n_tiles, int T, int32_t* __restrict__ tile_n) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_tiles) return;
  int n = 0;
  for (int r = 0; r < T; ++r) n += perm_pad[t * T + r] >= 0 ? 1 : 0;
  tile_n[t] = n;
}

// ---- pivots and workspace
// Two levels of pivots: C fine pivots (a cell of ~KNN_CELL points each) and C/16 coarse ones.  Points are ordered by
// (coarse pivot of their fine pivot, fine pivot), so that cells that follow each other in memory are neighbours in
// space and a 128-point tile that straddles two cells stays compact.
inline int64_t knn_coarse(int64_t C) { return C / 16 > 2 ? C / 16 : 2; }

inline int64_t knn_pivots(int64_t N) {
  // points per pivot.  Round 6 swept it (one box, GFICF_KNN_PIVOT_CELL): on 30 blobs in 50 dimensions larger cells win from 400 k points on
  // (400 k: 36.8 ms at 256, 28.0 at 1024; 1 M: 303 / 207 / 186 ms at 244 / 1024 / 4096 — cells are padded to whole tiles and the per-tile
  // bounds grow with the number of cells), but a cell has to stay finer than the data's clusters: 1 M points in 200 clusters take 221 ms at
  // 256 and 2 358 ms at 1 953 (nothing left to prune: the plain form).  The size that is safe for both stays; bounds per cell first and per
  // tile inside the cells in reach would lift the cost that grows with the cells (not built: it would be a step of knn.hip's KnnRun
  // between bounds() and search_both_forms()).
  int64_t per = 256;
  if (const char* e = getenv("GFICF_KNN_PIVOT_CELL")) per = atoi(e) > 0 ? atoi(e) : per;    // lab knob: points per pivot
  int64_t c = gficf_ceil_div(N, per);
  return c < 2 ? 2 : c > 4096 ? 4096 : c;
}

// workspace of the pruned search, carved in this order.  Rows / tiles are counted with the padding of the cell-aligned
// layout at its worst (every cell adds less than one tile).
struct KnnPruneWs {
  int64_t C, xrows, qrows, n_ct, n_qt;      // pivots; padded candidate / query rows; candidate / query tiles (upper bounds)
  float *pivots, *coarse, *xp, *qp, *centers, *radius, *lb;
  u64* apart;                       // assignment: N lists of one key (also used for the pivots' own assignment)
  int32_t *pivot_of, *coarse_of, *key_tmp, *perm_sorted, *perm_x, *perm_q, *cstart, *pstart, *tile_n, *qtile_n;
  int64_t* rank;
  u64 *kv0, *kv1;                   // the cell sort: its elements (N each) and its digit counts
  int64_t* hist;
  u64* part;
  u64* part_plain;                  // the plain search's partial lists (taken when the data does not prune)
  unsigned long long* counters;     // [0] zero-bound pairs, [1] pairs, [2] (as uint32) the choice flag
  size_t total;
};

inline KnnPruneWs knn_prune_ws(char* base, int64_t n_q, int64_t N, int dpad, int k) {
  KnnPruneWs w{};
  gficf_carver cv{base};
  const int64_t C = knn_pivots(N);
  w.C = C;
  w.n_ct = gficf_ceil_div(N, KNN_TC) + (C < N ? C : N);
  w.n_qt = gficf_ceil_div(n_q, KNN_TQ) + (C < n_q ? C : n_q);
  w.xrows = w.n_ct * KNN_TC;
  w.qrows = w.n_qt * KNN_TQ;
  w.pivots = cv.take<float>((size_t)C * dpad);
  w.coarse = cv.take<float>((size_t)knn_coarse(C) * dpad);
  w.coarse_of = cv.take<int32_t>((size_t)C);
  w.xp = cv.take<float>((size_t)w.xrows * dpad);
  w.qp = cv.take<float>((size_t)w.qrows * dpad);
  w.centers = cv.take<float>((size_t)w.n_ct * dpad);
  w.radius = cv.take<float>((size_t)w.n_ct);
  w.lb = cv.take<float>((size_t)w.n_qt * w.n_ct);
  w.apart = cv.take<u64>((size_t)N);
  w.pivot_of = cv.take<int32_t>((size_t)N);
  w.key_tmp = cv.take<int32_t>((size_t)N);
  w.perm_sorted = cv.take<int32_t>((size_t)N);
  w.perm_x = cv.take<int32_t>((size_t)w.xrows);
  w.perm_q = cv.take<int32_t>((size_t)w.qrows);
  w.cstart = cv.take<int32_t>((size_t)(C + 2));
  w.pstart = cv.take<int32_t>((size_t)(C + 2));
  w.tile_n = cv.take<int32_t>((size_t)w.n_ct);
  w.qtile_n = cv.take<int32_t>((size_t)w.n_qt);
  w.rank = cv.take<int64_t>((size_t)(N + 1));
  w.kv0 = cv.take<u64>((size_t)N);
  w.kv1 = cv.take<u64>((size_t)N);
  w.hist = cv.take<int64_t>((size_t)gficf_radix_sort_hist_len(N, KNN_CELL_KEY_BITS));
  w.part = cv.take<u64>((size_t)w.qrows * (size_t)k);
  w.part_plain = cv.take<u64>((size_t)n_q * (size_t)KNN_MAX_SPLIT * (size_t)k);
  w.counters = cv.take<unsigned long long>(4);
  w.total = cv.total();
  return w;
}

}  // namespace
