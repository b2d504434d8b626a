// tsne.hip — the "tsne" reduction of the reference (R/dimensinalityReduction.R:175-177 through Rtsne::Rtsne): perplexity graph,
// exact repulsion, gradient descent with gains and momentum.  Built into libgficf_tsne.so, which links libgficf_hip.so and uses
// its context, pool, neighbour search, radix sort, scan and error plumbing (include/gficf_tsne.h states the algorithm, the
// arithmetic and what is relaxed).
//
// Launches of the affinity stage (N points, K = k - 1 columns, M = 2 N K items: every conditional once as (i, j), once as (j, i)):
//   k_ts_beta        one lane per point: the bisection for beta in f64, the K conditionals; bad ids and distances flagged
//   (knn_symmetrise.h)   the items sorted by (row, column), a pair combined by ts_combine, the kept entries emitted as CSR
// Launches of one evaluation of the gradient:
//   k_ts_repulse     the hot kernel.  Grid (row blocks, slices).  A lane owns TS_R = 2 rows i (y_i and three f32 accumulators
//                    each in registers); the workgroup walks its slice of j in tiles of 128 positions staged in LDS and read
//                    back as broadcasts (the j loop is wave-uniform).  Per pair and row: 2 sub, 2 fma, 1 rcp, 1 mul, 1 add,
//                    2 fma.  After every tile the f32 sums go into f64 accumulators; a workgroup writes (rep_x, rep_y) per row
//                    and slice, and one f64 z for all its rows (fixed tree).
//   k_ts_update      row-local, 8 lanes per row: Z (every workgroup adds the z of all (row block, slice) in the same order),
//                    the attractive walk over the row of P in f64, the slices of rep in order, dC; in the layout also gains,
//                    velocity, the move into the second buffer and the workgroup's partial column sums.  <.., KL>: the row's
//                    share of the KL divergence.
// and of the layout, per iteration: k_ts_repulse, k_ts_update, k_ts_centre (every workgroup adds the partial column sums in the
// same order and subtracts the means from its rows, back into Y).
#include <cmath>
#include <vector>

#include "addon_kernels.h"
#include "addon_status.h"
#include "block_ops.h"
#include "common.h"
#include "gficf_tsne.h"
#include "knn_symmetrise.h"

namespace {

constexpr int TS_TILE = GFICF_TSNE_TILE;     // positions j per LDS tile = the longest f32 accumulation chain
constexpr int TS_R = 2;                      // rows per lane of the repulsion kernel
constexpr int TS_ROWS = 256 * TS_R;          // rows per workgroup of the repulsion kernel
constexpr int TS_BLOCKS = 1024;              // workgroups the repulsion grid is cut towards (a constant: the shape depends on N only)
constexpr int TS_GROUP = 8;                  // lanes per row of the update kernel
constexpr int TS_UROWS = 256 / TS_GROUP;     // rows per workgroup of the update kernel
constexpr int TS_MAX_STEPS = 200;            // evaluations of the bisection
constexpr uint32_t TS_ST_ID = GFICF_AST_ID;          // a neighbour id outside [1, N], a column of P outside [0, N)
constexpr uint32_t TS_ST_VALUE = GFICF_AST_VALUE;    // a non-finite distance or coordinate, a bad value of P
constexpr uint32_t TS_ST_CSC = GFICF_AST_CSC;        // a row pointer of P that decreases or leaves [0, capacity]

unsigned ts_grid(int64_t n) { return (unsigned)gficf_ceil_div(n > 0 ? n : 1, 256); }

struct TsShape { int64_t row_blocks, tiles_per_slice, slices; };

TsShape ts_shape(int64_t N) {
  TsShape s;
  s.row_blocks = gficf_ceil_div(N, TS_ROWS);
  const int64_t tiles = gficf_ceil_div(N, TS_TILE);
  int64_t want = gficf_ceil_div(TS_BLOCKS, s.row_blocks);
  if (want > tiles) want = tiles;
  if (want > 65535) want = 65535;
  s.tiles_per_slice = gficf_ceil_div(tiles, want);
  s.slices = gficf_ceil_div(tiles, s.tiles_per_slice);            // no empty slice
  return s;
}

// the sum of n values: lane t adds the values t, t + 256, .. in order, then the fixed tree of block_ops.h
__device__ inline double ts_strided_sum(const double* __restrict__ v, int64_t n, double* sh) {
  double s = 0.0;
  for (int64_t t = threadIdx.x; t < n; t += 256) s += v[t];
  return gficf_block_sum_f64(s, sh);
}

// ------------------------------------------------------------------------------------------------ affinities: beta, Pc
__global__ __launch_bounds__(256) void k_ts_beta(const int32_t* __restrict__ idx, const float* __restrict__ dist, int64_t N, int K, int64_t ld,
                                                 double log_perp, float* __restrict__ W, double* __restrict__ beta_out,
                                                 uint32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  bool bad_id = false, bad_val = false;
  double dmin = INFINITY;
  for (int c = 0; c <= K; ++c) {
    const int32_t j = idx[(int64_t)c * ld + i];
    const float d = dist[(int64_t)c * ld + i];
    bad_val |= !isfinite(d);
    const bool in = j >= 1 && (int64_t)j <= N;
    bad_id |= !in;
    if (c >= 1 && in && (int64_t)j - 1 != i) dmin = fmin(dmin, (double)d * (double)d);
  }
  if (bad_id) atomicOr(status, TS_ST_ID);
  if (bad_val) atomicOr(status, TS_ST_VALUE);
  double beta = 1.0, lo = -INFINITY, hi = INFINITY, sum = 0.0;
  for (int it = 0; it < TS_MAX_STEPS; ++it) {
    double dsum = 0.0;
    sum = 0.0;
    for (int c = 1; c <= K; ++c) {
      const int32_t j = idx[(int64_t)c * ld + i];
      if (j < 1 || (int64_t)j > N || (int64_t)j - 1 == i) continue;
      const double d = (double)dist[(int64_t)c * ld + i], x = d * d - dmin, p = exp(-beta * x);
      sum += p;
      dsum += x * p;
    }
    const double diff = beta * dsum / sum + log(sum) - log_perp;
    if (fabs(diff) < 1e-5 || it == TS_MAX_STEPS - 1) break;
    if (diff > 0.0) {
      lo = beta;
      beta = isinf(hi) ? beta * 2.0 : (beta + hi) * 0.5;
    } else {
      hi = beta;
      beta = isinf(lo) ? beta * 0.5 : (beta + lo) * 0.5;
    }
  }
  if (beta_out) beta_out[i] = beta;
  for (int c = 1; c <= K; ++c) {
    const int32_t j = idx[(int64_t)c * ld + i];
    float w = 0.f;
    if (j >= 1 && (int64_t)j <= N && (int64_t)j - 1 != i) {
      const double d = (double)dist[(int64_t)c * ld + i];
      w = (float)(exp(-beta * (d * d - dmin)) / sum);
    }
    W[(int64_t)(c - 1) * N + i] = w > 0.f ? w : 0.f;             // (a NaN distance, flagged above, leaves no entry)
  }
}

// ------------------------------------------------------------------------------------------------ affinities: symmetrisation
// the two conditionals of a pair, smaller first: both directions evaluate the same expression on the same operands
struct ts_combine {
  double two_n;
  __device__ float operator()(float x, float y) const {
    const float lo = fminf(x, y), hi = fmaxf(x, y);
    return (float)(((double)lo + (double)hi) / two_n);
  }
};

// ------------------------------------------------------------------------------------------------ gradient: checks
// one lane per row and per entry of P and per coordinate, whichever is more
__global__ __launch_bounds__(256) void k_ts_check(int64_t N, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                  const float* __restrict__ val, int64_t cap, const float* __restrict__ Y,
                                                  uint32_t* __restrict__ status) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t st = 0u;
  if (t < N) {
    const int64_t b = rowptr[t], e = rowptr[t + 1];
    if (b < 0 || e < b || e > cap || (t == 0 && b != 0)) st |= TS_ST_CSC;
  }
  if (t < 2 * N && !isfinite(Y[t])) st |= TS_ST_VALUE;
  if (t < gficf_addon_nnz(rowptr, N, cap)) {
    const int32_t j = col[t];
    const float w = val[t];
    if (j < 0 || (int64_t)j >= N) st |= TS_ST_ID;
    if (!(w >= 0.f) || isinf(w)) st |= TS_ST_VALUE;
  }
  if (st) atomicOr(status, st);
}

// ------------------------------------------------------------------------------------------------ gradient: the repulsive field
// one pair: the contract's operation list (include/gficf_tsne.h); fmaf is written out, the file is built with -ffp-contract=off
__device__ inline void ts_pair(float yx, float yy, float2 p, float& rx, float& ry, float& z) {
  const float dx = yx - p.x, dy = yy - p.y;
  const float q = __builtin_amdgcn_rcpf(fmaf(dx, dx, fmaf(dy, dy, 1.f)));
  const float q2 = q * q;
  z += q;
  rx = fmaf(q2, dx, rx);
  ry = fmaf(q2, dy, ry);
}

__global__ __launch_bounds__(256) void k_ts_repulse(const float2* __restrict__ Y, int64_t N, int64_t tiles_per_slice, double* __restrict__ part,
                                                    double* __restrict__ zpart) {
  __shared__ __attribute__((aligned(16))) float2 sh[TS_TILE];
  __shared__ double red[256];
  const int64_t rb = blockIdx.x, s = blockIdx.y;
  int64_t row[TS_R];
  float yx[TS_R], yy[TS_R];
  double ax[TS_R], ay[TS_R], az[TS_R];
#pragma unroll
  for (int r = 0; r < TS_R; ++r) {
    row[r] = rb * TS_ROWS + (int64_t)r * 256 + threadIdx.x;
    const float2 y = row[r] < N ? Y[row[r]] : make_float2(0.f, 0.f);
    yx[r] = y.x; yy[r] = y.y;
    ax[r] = ay[r] = az[r] = 0.0;
  }
  const int64_t j_begin = s * tiles_per_slice * TS_TILE;
  int64_t j_end = j_begin + tiles_per_slice * TS_TILE;
  if (j_end > N) j_end = N;
  for (int64_t jb = j_begin; jb < j_end; jb += TS_TILE) {
    const int cnt = j_end - jb < TS_TILE ? (int)(j_end - jb) : TS_TILE;
    __syncthreads();                                            // the previous tile has been read
    if ((int)threadIdx.x < cnt) sh[threadIdx.x] = Y[jb + threadIdx.x];
    __syncthreads();
    float rx[TS_R], ry[TS_R], z[TS_R];
#pragma unroll
    for (int r = 0; r < TS_R; ++r) rx[r] = ry[r] = z[r] = 0.f;
    if (cnt == TS_TILE) {
#pragma unroll 8
      for (int t = 0; t < TS_TILE; ++t) {
        const float2 p = sh[t];
#pragma unroll
        for (int r = 0; r < TS_R; ++r) ts_pair(yx[r], yy[r], p, rx[r], ry[r], z[r]);
      }
    } else {
      for (int t = 0; t < cnt; ++t) {
        const float2 p = sh[t];
#pragma unroll
        for (int r = 0; r < TS_R; ++r) ts_pair(yx[r], yy[r], p, rx[r], ry[r], z[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < TS_R; ++r) {
      ax[r] += (double)rx[r]; ay[r] += (double)ry[r]; az[r] += (double)z[r];
    }
  }
  double zl = 0.0;
#pragma unroll
  for (int r = 0; r < TS_R; ++r) {
    if (row[r] < N) {
      double* o = part + 2 * (s * N + row[r]);
      o[0] = ax[r]; o[1] = ay[r];
      zl += az[r];
    }
  }
  const double zb = gficf_block_sum_f64(zl, red);
  if (threadIdx.x == 0) zpart[rb * gridDim.y + s] = zb;
}

// ------------------------------------------------------------------------------------------------ gradient: the row-local half
struct TsUp {
  int64_t N, cap, slices, nz;
  const int64_t* rowptr;
  const int32_t* col;
  const float* val;
  const float2* Y;
  const double* part;
  const double* zpart;
  double x;                       // the exaggeration in force
  float2* dC;                     // outputs of the gradient entry (each may be NULL)
  float2* rep;
  double* Z;
  double* klpart;
  float2 *uY, *gains, *Ynew;      // the layout's state and its second buffer
  double* ypart;
  float mu, eta;
};

__device__ inline float ts_sign(float v) { return v > 0.f ? 1.f : v < 0.f ? -1.f : 0.f; }

__device__ inline void ts_step(float dc, float& gain, float& u, float& y, float mu, float eta) {
  gain = ts_sign(dc) != ts_sign(u) ? gain + 0.2f : gain * 0.8f;
  gain = fmaxf(gain, 0.01f);
  u = mu * u - (eta * gain) * dc;
  y = y + u;
}

template <bool LAYOUT, bool KL>
__global__ __launch_bounds__(256) void k_ts_update(TsUp U) {
  __shared__ double red[256];
  __shared__ double sx[TS_UROWS], sy[TS_UROWS], sk[TS_UROWS];
  const double Z = ts_strided_sum(U.zpart, U.nz, red) - (double)U.N;        // the j = i pairs, one each
  if (blockIdx.x == 0 && threadIdx.x == 0 && U.Z) *U.Z = Z;
  const int g = threadIdx.x / TS_GROUP, lane = threadIdx.x % TS_GROUP;
  const int64_t row = (int64_t)blockIdx.x * TS_UROWS + g;
  const bool valid = row < U.N;
  double ax = 0.0, ay = 0.0, kl = 0.0;
  float2 yi = make_float2(0.f, 0.f);
  if (valid) {
    int64_t e0 = U.rowptr[row], e1 = U.rowptr[row + 1];
    if (e0 < 0) e0 = 0;
    if (e1 > U.cap) e1 = U.cap;
    yi = U.Y[row];
    for (int64_t e = e0 + lane; e < e1; e += TS_GROUP) {
      const int32_t j = U.col[e];
      if (j < 0 || (int64_t)j >= U.N) continue;
      const double p = (double)U.val[e];
      const float2 yj = U.Y[j];
      const double dx = (double)yi.x - (double)yj.x, dy = (double)yi.y - (double)yj.y, s = 1.0 + (dx * dx + dy * dy), pq = p / s;
      ax += pq * dx;
      ay += pq * dy;
      if (KL && p > 0.0) kl += p * log(p * Z * s);
    }
  }
  for (int m = TS_GROUP / 2; m >= 1; m >>= 1) {                 // the same tree in every lane of the group
    ax += __shfl_xor(ax, m, TS_GROUP);
    ay += __shfl_xor(ay, m, TS_GROUP);
    if (KL) kl += __shfl_xor(kl, m, TS_GROUP);
  }
  double nx = 0.0, ny = 0.0;
  if (valid && lane == 0) {
    double rx = 0.0, ry = 0.0;
    for (int64_t s = 0; s < U.slices; ++s) {
      const double* o = U.part + 2 * (s * U.N + row);
      rx += o[0]; ry += o[1];
    }
    const double zi = Z > 0.0 ? 1.0 / Z : 0.0;
    const float dcx = (float)(U.x * ax - rx * zi), dcy = (float)(U.x * ay - ry * zi);
    if (U.dC) U.dC[row] = make_float2(dcx, dcy);
    if (U.rep) U.rep[row] = make_float2((float)rx, (float)ry);
    if (LAYOUT) {
      float2 gn = U.gains[row], u = U.uY[row], y = yi;
      ts_step(dcx, gn.x, u.x, y.x, U.mu, U.eta);
      ts_step(dcy, gn.y, u.y, y.y, U.mu, U.eta);
      U.gains[row] = gn;
      U.uY[row] = u;
      U.Ynew[row] = y;
      nx = (double)y.x; ny = (double)y.y;
    }
  }
  if (lane == 0) { sx[g] = nx; sy[g] = ny; sk[g] = valid ? kl : 0.0; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tx = 0.0, ty = 0.0, tk = 0.0;
    for (int r = 0; r < TS_UROWS; ++r) { tx += sx[r]; ty += sy[r]; tk += sk[r]; }
    if (LAYOUT) { U.ypart[2 * (int64_t)blockIdx.x] = tx; U.ypart[2 * (int64_t)blockIdx.x + 1] = ty; }
    if (KL) U.klpart[blockIdx.x] = tk;
  }
}

// ypart: the partial column sums (x, y) of the nparts workgroups of k_ts_update
__global__ __launch_bounds__(256) void k_ts_centre(const float2* __restrict__ Ynew, float2* __restrict__ Y, int64_t N,
                                                   const double* __restrict__ ypart, int64_t nparts) {
  __shared__ double red[256];
  double sx = 0.0, sy = 0.0;
  for (int64_t t = threadIdx.x; t < nparts; t += 256) { sx += ypart[2 * t]; sy += ypart[2 * t + 1]; }
  const double mx = gficf_block_sum_f64(sx, red) / (double)N, my = gficf_block_sum_f64(sy, red) / (double)N;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const float2 y = Ynew[i];
  Y[i] = make_float2((float)((double)y.x - mx), (float)((double)y.y - my));
}

__global__ __launch_bounds__(256) void k_ts_kl_fin(const double* __restrict__ klpart, int64_t nparts, double* __restrict__ kl) {
  __shared__ double red[256];
  const double s = ts_strided_sum(klpart, nparts, red);
  if (threadIdx.x == 0) *kl = s;
}

// ------------------------------------------------------------------------------------------------ boundary conversions (chain)
__global__ __launch_bounds__(256) void k_ts_in(const double* __restrict__ init, int64_t N, float* __restrict__ Y, float* __restrict__ uY,
                                               float* __restrict__ gains) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= 2 * N) return;
  Y[t] = (float)init[(t & 1) * N + (t >> 1)];                   // (a non-finite one is flagged by the layout's check)
  uY[t] = 0.f;
  gains[t] = 1.f;
}

// ------------------------------------------------------------------------------------------------ workspaces
struct TsAffWs {
  uint32_t* status;
  float* W;
  SymWs sym;
};

size_t ts_carve_aff(char* base, int64_t N, int K, TsAffWs& w) {
  gficf_carver cv;
  cv.base = base;
  w.status = cv.take<uint32_t>(1);
  w.W = cv.take<float>((size_t)N * (size_t)K);
  sym_carve(cv, N, 2 * (size_t)N * (size_t)K, w.sym);
  return cv.total();
}

struct TsLayWs {
  uint32_t* status;
  float* Y1;                      // the second position buffer
  float* dC;                      // where the gradient goes when nobody asks for it
  double* part;                   // (rep_x, rep_y) per slice and row
  double* zpart;                  // z per (row block, slice)
  double* ypart;                  // partial column sums per workgroup of the update kernel
  double* klpart;
  double* Z;
};

size_t ts_carve_lay(char* base, int64_t N, TsLayWs& w) {
  gficf_carver cv;
  cv.base = base;
  const TsShape sh = ts_shape(N);
  const size_t ub = (size_t)gficf_ceil_div(N, TS_UROWS);
  w.status = cv.take<uint32_t>(1);
  w.Y1 = cv.take<float>(2 * (size_t)N);
  w.dC = cv.take<float>(2 * (size_t)N);
  w.part = cv.take<double>(2 * (size_t)N * (size_t)sh.slices);
  w.zpart = cv.take<double>((size_t)(sh.row_blocks * sh.slices));
  w.ypart = cv.take<double>(2 * ub);
  w.klpart = cv.take<double>(ub);
  w.Z = cv.take<double>(1);
  return cv.total();
}

int ts_check_aff(int64_t N, int k, int64_t ld, double perplexity) {
  if (N < 1) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "N = %lld: no points", (long long)N);
  if (!(perplexity > 0.0) || !std::isfinite(perplexity)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "perplexity = %g must be positive", perplexity);
  if (!((double)(N - 1) >= 3.0 * perplexity))
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "perplexity = %g is too large for N = %lld points (N - 1 >= 3 perplexity)", perplexity, (long long)N);
  if (std::floor(3.0 * perplexity) + 1.0 > (double)GFICF_KNN_MAX_K)
    GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "perplexity = %g needs %g neighbours, beyond %d", perplexity, std::floor(3.0 * perplexity) + 1.0,
               GFICF_KNN_MAX_K);
  if (k != (int)std::floor(3.0 * perplexity) + 1)
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "k = %d columns, perplexity = %g needs floor(3 perplexity) + 1 = %d", k, perplexity,
               (int)std::floor(3.0 * perplexity) + 1);
  if (k < 2) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "perplexity = %g names no neighbour (floor(3 perplexity) = 0)", perplexity);
  if (N * k >= ((int64_t)1 << 31)) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "N * k = %lld reaches 2^31", (long long)(N * k));
  if (ld < N) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "ld = %lld < N = %lld", (long long)ld, (long long)N);
  return GFICF_OK;
}

int ts_check_lay(int64_t N, int64_t cap, int max_iter, int ib, int ie, double momentum, double final_momentum, double eta, double exag) {
  if (N < 1 || N > 0x7FFFFFFFll) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "N = %lld outside [1, 2^31)", (long long)N);
  if (cap < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "negative capacity");
  if (max_iter < 0 || ib < 0 || ie < ib || ie > max_iter) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "iterations [%d, %d) of %d", ib, ie, max_iter);
  if (!std::isfinite(momentum) || !std::isfinite(final_momentum) || !std::isfinite(eta) || !std::isfinite(exag))
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "momentum / final_momentum / eta / exaggeration_factor not finite");
  return GFICF_OK;
}

// the affinity stage on a carved workspace whose status word the caller has zeroed
int ts_affinities(gficf_ctx* ctx, const TsAffWs& w, const int32_t* d_idx, const float* d_dist, int64_t N, int k, int64_t ld, double perplexity,
                  int64_t* d_rowptr, int32_t* d_col, float* d_val, int64_t* d_nnz, double* d_beta) {
  hipStream_t st = ctx->stream;
  const int K = k - 1;
  hipLaunchKernelGGL(k_ts_beta, dim3(ts_grid(N)), dim3(256), 0, st, d_idx, d_dist, N, K, ld, std::log(perplexity), w.W, d_beta, w.status);
  return sym_enqueue(ctx, w.sym, d_idx, 1, w.W, N, K, ld, ts_combine{2.0 * (double)N}, d_rowptr, d_col, d_val, d_nnz);
}

void ts_launch_check(hipStream_t st, const TsLayWs& w, int64_t N, const int64_t* d_rowptr, const int32_t* d_col, const float* d_val, int64_t cap,
                     const float* d_Y) {
  const int64_t n = cap > 2 * N ? cap : 2 * N;
  hipLaunchKernelGGL(k_ts_check, dim3(ts_grid(n)), dim3(256), 0, st, N, d_rowptr, d_col, d_val, cap, d_Y, w.status);
}

TsUp ts_up(const TsLayWs& w, int64_t N, const int64_t* d_rowptr, const int32_t* d_col, const float* d_val, int64_t cap) {
  const TsShape sh = ts_shape(N);
  TsUp U{};
  U.N = N; U.cap = cap; U.slices = sh.slices; U.nz = sh.row_blocks * sh.slices;
  U.rowptr = d_rowptr; U.col = d_col; U.val = d_val;
  U.part = w.part; U.zpart = w.zpart; U.klpart = w.klpart; U.ypart = w.ypart;
  U.x = 1.0;
  return U;
}

void ts_launch_repulse(hipStream_t st, const TsLayWs& w, int64_t N, const float* d_Y) {
  const TsShape sh = ts_shape(N);
  hipLaunchKernelGGL(k_ts_repulse, dim3((unsigned)sh.row_blocks, (unsigned)sh.slices), dim3(256), 0, st, (const float2*)d_Y, N, sh.tiles_per_slice,
                     w.part, w.zpart);
}

// one evaluation of the gradient at d_Y (no checks): dC, rep, Z, KL as asked for
int ts_gradient(gficf_ctx* ctx, const TsLayWs& w, int64_t N, const int64_t* d_rowptr, const int32_t* d_col, const float* d_val, int64_t cap,
                const float* d_Y, double x, float* d_dC, float* d_rep, double* d_Z, double* d_kl) {
  hipStream_t st = ctx->stream;
  const unsigned ub = (unsigned)gficf_ceil_div(N, TS_UROWS);
  ts_launch_repulse(st, w, N, d_Y);
  TsUp U = ts_up(w, N, d_rowptr, d_col, d_val, cap);
  U.Y = (const float2*)d_Y; U.x = x; U.dC = (float2*)d_dC; U.rep = (float2*)d_rep; U.Z = d_Z;
  if (d_kl) {
    hipLaunchKernelGGL((k_ts_update<false, true>), dim3(ub), dim3(256), 0, st, U);
    hipLaunchKernelGGL(k_ts_kl_fin, dim3(1), dim3(256), 0, st, (const double*)w.klpart, (int64_t)ub, d_kl);
  } else {
    hipLaunchKernelGGL((k_ts_update<false, false>), dim3(ub), dim3(256), 0, st, U);
  }
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

// the layout stage on a carved workspace whose status word the caller has zeroed
int ts_layout(gficf_ctx* ctx, const TsLayWs& w, int64_t N, const int64_t* d_rowptr, const int32_t* d_col, const float* d_val, int64_t cap, int ib,
              int ie, int stop_lying, int mom_switch, float momentum, float final_momentum, float eta, double exag, float* d_Y, float* d_uY,
              float* d_gains, double* d_kl) {
  hipStream_t st = ctx->stream;
  const unsigned ub = (unsigned)gficf_ceil_div(N, TS_UROWS);
  ts_launch_check(st, w, N, d_rowptr, d_col, d_val, cap, d_Y);
  TsUp U = ts_up(w, N, d_rowptr, d_col, d_val, cap);
  U.Y = (const float2*)d_Y; U.uY = (float2*)d_uY; U.gains = (float2*)d_gains; U.Ynew = (float2*)w.Y1; U.eta = eta;
  for (int n = ib; n < ie; ++n) {
    U.x = n < stop_lying ? exag : 1.0;
    U.mu = n < mom_switch ? momentum : final_momentum;
    ts_launch_repulse(st, w, N, d_Y);
    hipLaunchKernelGGL((k_ts_update<true, false>), dim3(ub), dim3(256), 0, st, U);
    hipLaunchKernelGGL(k_ts_centre, dim3(ts_grid(N)), dim3(256), 0, st, (const float2*)w.Y1, (float2*)d_Y, N, (const double*)w.ypart, (int64_t)ub);
  }
  GFICF_HIP_CHECK(hipGetLastError());
  if (d_kl) return ts_gradient(ctx, w, N, d_rowptr, d_col, d_val, cap, d_Y, 1.0, w.dC, nullptr, w.Z, d_kl);
  return GFICF_OK;
}

}  // namespace

extern "C" {

int gficf_tsne_abi_version(void) { return GFICF_TSNE_ABI_VERSION; }

size_t gficf_tsne_affinities_workspace_bytes(int64_t N, int k) {
  if (N < 1 || k < 2 || k > GFICF_KNN_MAX_K || N * k >= ((int64_t)1 << 31)) return 0;
  TsAffWs w;
  return ts_carve_aff(nullptr, N, k - 1, w);
}

int gficf_tsne_affinities_device(gficf_ctx* ctx, const int32_t* d_idx, const float* d_dist, int64_t N, int k, int64_t ld, double perplexity,
                                 void* ws, size_t ws_bytes, int64_t* d_rowptr, int32_t* d_col, float* d_val, int64_t capacity, int64_t* d_nnz,
                                 double* d_beta, float* d_pc) {
  GFICF_CTX_ENTER(ctx);
  const int rc = ts_check_aff(N, k, ld, perplexity);
  if (rc) return rc;
  if (!d_idx || !d_dist || !ws || !d_rowptr || !d_col || !d_val || !d_nnz) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  const int64_t need_cap = 2 * N * (k - 1);
  if (capacity < need_cap) GFICF_FAIL(GFICF_ERR_CAPACITY, "capacity %lld < 2 N K = %lld entries", (long long)capacity, (long long)need_cap);
  TsAffWs w;
  const size_t need = ts_carve_aff(nullptr, N, k - 1, w);
  if (ws_bytes < need) GFICF_FAIL(GFICF_ERR_CAPACITY, "workspace too small: %zu < %zu bytes", ws_bytes, need);
  ts_carve_aff((char*)ws, N, k - 1, w);
  GFICF_HIP_CHECK(hipMemsetAsync(w.status, 0, sizeof(uint32_t), ctx->stream));
  const int ra = ts_affinities(ctx, w, d_idx, d_dist, N, k, ld, perplexity, d_rowptr, d_col, d_val, d_nnz, d_beta);
  if (ra) return ra;
  if (d_pc) GFICF_HIP_CHECK(hipMemcpyAsync(d_pc, w.W, sizeof(float) * (size_t)N * (size_t)(k - 1), hipMemcpyDeviceToDevice, ctx->stream));
  return GFICF_OK;
}

int gficf_tsne_shape(int64_t N, int* rows_per_block, int* tile, int* slices) {
  if (N < 1 || N > 0x7FFFFFFFll) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "N = %lld outside [1, 2^31)", (long long)N);
  const TsShape sh = ts_shape(N);
  if (rows_per_block) *rows_per_block = TS_ROWS;
  if (tile) *tile = TS_TILE;
  if (slices) *slices = (int)sh.slices;
  return GFICF_OK;
}

size_t gficf_tsne_layout_workspace_bytes(int64_t N, int64_t capacity) {
  if (N < 1 || N > 0x7FFFFFFFll || capacity < 0) return 0;
  TsLayWs w;
  return ts_carve_lay(nullptr, N, w);
}

int gficf_tsne_gradient_device(gficf_ctx* ctx, int64_t N, const int64_t* d_rowptr, const int32_t* d_col, const float* d_val, int64_t capacity,
                               const float* d_Y, double exaggeration, void* ws, size_t ws_bytes, float* d_dC, float* d_rep, double* d_Z,
                               double* d_kl) {
  GFICF_CTX_ENTER(ctx);
  const int rc = ts_check_lay(N, capacity, 0, 0, 0, 0.0, 0.0, 0.0, exaggeration);
  if (rc) return rc;
  if (!d_rowptr || !d_Y || !ws || !d_dC || !d_Z || (capacity > 0 && (!d_col || !d_val))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  TsLayWs w;
  const size_t need = ts_carve_lay(nullptr, N, w);
  if (ws_bytes < need) GFICF_FAIL(GFICF_ERR_CAPACITY, "workspace too small: %zu < %zu bytes", ws_bytes, need);
  ts_carve_lay((char*)ws, N, w);
  GFICF_HIP_CHECK(hipMemsetAsync(w.status, 0, sizeof(uint32_t), ctx->stream));
  ts_launch_check(ctx->stream, w, N, d_rowptr, d_col, d_val, capacity, d_Y);
  return ts_gradient(ctx, w, N, d_rowptr, d_col, d_val, capacity, d_Y, exaggeration, d_dC, d_rep, d_Z, d_kl);
}

int gficf_tsne_layout_device(gficf_ctx* ctx, int64_t N, const int64_t* d_rowptr, const int32_t* d_col, const float* d_val, int64_t capacity,
                             int max_iter, int iter_begin, int iter_end, int stop_lying_iter, int mom_switch_iter, double momentum,
                             double final_momentum, double eta, double exaggeration_factor, float* d_Y, float* d_uY, float* d_gains, void* ws,
                             size_t ws_bytes, double* d_kl) {
  GFICF_CTX_ENTER(ctx);
  const int rc = ts_check_lay(N, capacity, max_iter, iter_begin, iter_end, momentum, final_momentum, eta, exaggeration_factor);
  if (rc) return rc;
  if (!d_rowptr || !d_Y || !d_uY || !d_gains || !ws || (capacity > 0 && (!d_col || !d_val))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  TsLayWs w;
  const size_t need = ts_carve_lay(nullptr, N, w);
  if (ws_bytes < need) GFICF_FAIL(GFICF_ERR_CAPACITY, "workspace too small: %zu < %zu bytes", ws_bytes, need);
  ts_carve_lay((char*)ws, N, w);
  GFICF_HIP_CHECK(hipMemsetAsync(w.status, 0, sizeof(uint32_t), ctx->stream));
  return ts_layout(ctx, w, N, d_rowptr, d_col, d_val, capacity, iter_begin, iter_end, stop_lying_iter, mom_switch_iter, (float)momentum,
                   (float)final_momentum, (float)eta, exaggeration_factor, d_Y, d_uY, d_gains, d_kl);
}

int gficf_tsne_sync(gficf_ctx* ctx, const void* ws) {
  uint32_t st;
  const int rc = gficf_addon_read_status(ctx, ws, &st);
  if (rc) return rc;
  if (st & TS_ST_ID) GFICF_FAIL(GFICF_ERR_BAD_ID, "a neighbour id outside [1, N] or a column of P outside [0, N)");
  if (st & TS_ST_CSC) GFICF_FAIL(GFICF_ERR_BAD_CSC, "a row pointer of P decreases or leaves [0, capacity]");
  if (st & TS_ST_VALUE) GFICF_FAIL(GFICF_ERR_BAD_VALUE, "a non-finite distance or coordinate, or a value of P that is negative or not finite");
  return GFICF_OK;
}

int gficf_tsne_host(gficf_ctx* ctx, const double* X, int64_t N, int d, int64_t ld, double perplexity, int max_iter, int stop_lying_iter,
                    int mom_switch_iter, double momentum, double final_momentum, double eta, double exaggeration_factor, const double* init,
                    double* embedding, double* kl, int64_t* rowptr, int32_t* col, float* val, int64_t* nnz, int32_t* idx, float* dist) {
  GFICF_CTX_ENTER(ctx);
  if (!(perplexity > 0.0) || !std::isfinite(perplexity)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "perplexity = %g must be positive", perplexity);
  const double kd = std::floor(3.0 * perplexity) + 1.0;
  const int k = kd > (double)GFICF_KNN_MAX_K ? GFICF_KNN_MAX_K + 1 : (int)kd;
  int rc = ts_check_aff(N, k, ld, perplexity);
  if (rc) return rc;
  const int64_t cap = 2 * N * (k - 1);
  rc = ts_check_lay(N, cap, max_iter, 0, max_iter, momentum, final_momentum, eta, exaggeration_factor);
  if (rc) return rc;
  if (d < 1 || gficf_knn_dpad(d) < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "d = %d outside [1, 128]", d);
  if (!X || !init || !embedding) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  const bool want_p = rowptr || col || val || nnz;
  if (want_p && (!rowptr || !col || !val || !nnz)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "P is returned whole: rowptr, col, val and nnz");
  const size_t nk = (size_t)N * (size_t)k, dpad = (size_t)gficf_knn_dpad(d);
  const size_t knn_b = gficf_knn_workspace_bytes(ctx, N, N, k), af_b = gficf_tsne_affinities_workspace_bytes(N, k),
               ly_b = gficf_tsne_layout_workspace_bytes(N, cap);
  TsAffWs aw;
  TsLayWs lw;
  gficf_host_io io{ctx, "gficf_tsne_host"};
  gficf_carver cv;
  double *d_X, *d_init, *d_emb, *d_kl; float *d_pts, *d_dist, *d_val, *d_Y, *d_uY, *d_gains; int32_t *d_idx, *d_col; int64_t *d_rowptr, *d_nnz;
  char *d_kws, *d_aws, *d_lws;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    d_lws = cv.take<char>(ly_b);                                // first: its head is the status word of the whole chain
    d_X = cv.take<double>((size_t)ld * (size_t)d); d_init = cv.take<double>(2 * (size_t)N); d_emb = cv.take<double>(2 * (size_t)N);
    d_kl = cv.take<double>(1);
    d_pts = cv.take<float>((size_t)N * dpad); d_idx = cv.take<int32_t>(nk); d_dist = cv.take<float>(nk);
    d_rowptr = cv.take<int64_t>((size_t)N + 1); d_col = cv.take<int32_t>((size_t)cap); d_val = cv.take<float>((size_t)cap);
    d_nnz = cv.take<int64_t>(1); d_Y = cv.take<float>(2 * (size_t)N); d_uY = cv.take<float>(2 * (size_t)N);
    d_gains = cv.take<float>(2 * (size_t)N);
    d_kws = cv.take<char>(knn_b); d_aws = cv.take<char>(af_b);
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_STAGE0);
  }
  io.up(d_X, X, sizeof(double) * (size_t)ld * (size_t)d);
  io.up(d_init, init, sizeof(double) * 2 * (size_t)N);
  int64_t h_nnz = 0;
  if (io.ok()) {
    hipStream_t st = ctx->stream;
    ts_carve_aff(d_aws, N, k - 1, aw);
    ts_carve_lay(d_lws, N, lw);
    aw.status = lw.status;                                      // one status word: what gficf_tsne_sync(ctx, d_lws) reads
    io.e = hipMemsetAsync(lw.status, 0, sizeof(uint32_t), st);
    if (io.ok()) {
      rc = gficf_knn_prepare_device(ctx, d_X, 1, N, d, ld, GFICF_KNN_EUCLIDEAN, d_pts);
      if (!rc) rc = gficf_knn_search_device(ctx, d_pts, N, d, k, GFICF_KNN_EUCLIDEAN, 0, N, d_kws, knn_b, d_idx, d_dist, N);
      if (!rc) rc = ts_affinities(ctx, aw, d_idx, d_dist, N, k, N, perplexity, d_rowptr, d_col, d_val, d_nnz, nullptr);
      if (!rc) {
        hipLaunchKernelGGL(k_ts_in, dim3(ts_grid(2 * N)), dim3(256), 0, st, (const double*)d_init, N, d_Y, d_uY, d_gains);
        rc = ts_layout(ctx, lw, N, d_rowptr, d_col, d_val, cap, 0, max_iter, stop_lying_iter, mom_switch_iter, (float)momentum,
                       (float)final_momentum, (float)eta, exaggeration_factor, d_Y, d_uY, d_gains, kl ? d_kl : nullptr);
      }
      if (!rc) {
        hipLaunchKernelGGL(k_addon_out, dim3(ts_grid(2 * N)), dim3(256), 0, st, (const float*)d_Y, N, d_emb);
        io.e = hipGetLastError();
        io.down(embedding, d_emb, sizeof(double) * 2 * (size_t)N);
        if (kl) io.down(kl, d_kl, sizeof(double));
        if (idx) io.down(idx, d_idx, sizeof(int32_t) * nk);
        if (dist) io.down(dist, d_dist, sizeof(float) * nk);
        if (want_p) {
          io.down(rowptr, d_rowptr, sizeof(int64_t) * ((size_t)N + 1));
          io.down(&h_nnz, d_nnz, sizeof(int64_t));
        }
      }
    }
  }
  if (!io.ok() || rc) return io.drain(rc);
  rc = gficf_tsne_sync(ctx, d_lws);
  if (rc) return rc;
  if (want_p) {                                                 // the entries in use only (their count has just arrived)
    *nnz = h_nnz;
    io.down(col, d_col, sizeof(int32_t) * (size_t)h_nnz);
    io.down(val, d_val, sizeof(float) * (size_t)h_nnz);
    return io.finish(GFICF_OK);
  }
  return GFICF_OK;
}

}  // extern "C"
