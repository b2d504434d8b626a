// hvg.hip — the highly variable genes of findVarGenes() (reference R/deGenes.R:72-164, scVEGs) from the sparse matrix: per-gene
// moments, the robust local regression of log10 cv on log10 mean, the trusted range and the curve through it, every gene's
// signed distance to the curve, the mode of the distances and their p-values.  Built into libgficf_hvg.so, which links
// libgficf_hip.so and uses its context, pool, radix sort, transpose and error plumbing (include/gficf_hvg.h states the contract).
//
// Launches, all on the context's stream:
//   (transpose)       gene-major view of the CSC input (gficf_csc_transpose_device)
//   k_hv_moments      one wave per gene: nobs, mean, the two-pass sum of squares, lx, ly, valid
//   k_hv_logs         the same lx, ly, valid from given mean and cv
//   (addon_sort.h: k_sort_keys, k_sort_next<0>, radix sort x 2), k_hv_perm   the stable order of a list of doubles, the
//                     invalid ones last
//   k_hv_gather       a list in that order
//   k_hv_sorted       the check that a list handed in as ascending is
//   k_hv_locfit       one wave per evaluation point: the window by binary search, eight wave sums, the 3 x 3 solve
//   k_hv_res, k_hv_median, k_hv_bisquare   a round of Cleveland's loop
//   k_hv_gap          one thread per grid point: two searches
//   k_hv_curve        the curve on the fine grid
//   k_hv_dist         one wave per gene: its window of the fine grid, the first minimum, the sign
//   k_hv_kde_stats    one workgroup: sd, quartiles, bandwidth, grid ends
//   k_hv_kde_dens     one workgroup per grid point: the folded sum of the Gaussian terms
//   k_hv_kde_mode     one workgroup: the first maximum
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "addon_sort.h"
#include "addon_status.h"
#include "common.h"
#include "gficf_hvg.h"

namespace {

constexpr uint32_t HV_ST_ORDER = 1u;                       // a list handed in as ascending decreases (or holds a NaN)

__device__ inline void hv_logs(double mean, double cv, double* lx, double* ly, int32_t* valid, int64_t g) {
  const double a = log10(mean), b = log10(cv);
  lx[g] = a;
  ly[g] = b;
  valid[g] = (isfinite(a) && isfinite(b)) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_hv_moments(int64_t G, int64_t N, int64_t nnz, const int64_t* __restrict__ tptr, const double* __restrict__ tx,
                                                    double* __restrict__ mean, double* __restrict__ sd, double* __restrict__ var,
                                                    int32_t* __restrict__ nobs, double* __restrict__ lx, double* __restrict__ ly,
                                                    int32_t* __restrict__ valid) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (g >= G) return;                                      // the whole wave
  int64_t beg = tptr[g], end = tptr[g + 1];
  if (beg < 0) beg = 0;                                    // (offsets a malformed CSC left: BAD_CSC is raised by the transpose)
  if (end > nnz) end = nnz;
  double a = 0.0;
  int cnt = 0;
  for (int64_t p = beg + lane; p < end; p += 64) {
    const double v = tx[p];
    if (v != 0.0) { a += v; ++cnt; }
  }
  a = gficf_wave_sum(a);
  cnt = gficf_wave_sum(cnt);
  const double m = a / (double)N;
  double b = 0.0;
  for (int64_t p = beg + lane; p < end; p += 64) {
    const double v = tx[p];
    if (v != 0.0) { const double d = v - m; b += d * d; }
  }
  b = gficf_wave_sum(b);
  const double ss = b + (double)(N - cnt) * (m * m);
  const double vr = ss / (double)(N - 1), s = sqrt(vr);
  if (lane == 0) {
    mean[g] = m;
    sd[g] = s;
    var[g] = vr;
    nobs[g] = cnt;
    hv_logs(m, s / m, lx, ly, valid, g);
  }
}

__global__ __launch_bounds__(256) void k_hv_logs(int64_t G, const double* __restrict__ mean, const double* __restrict__ cv, double* __restrict__ lx,
                                                 double* __restrict__ ly, int32_t* __restrict__ valid) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g < G) hv_logs(mean[g], cv[g], lx, ly, valid, g);
}

__global__ __launch_bounds__(256) void k_hv_perm(int64_t n, const uint32_t* __restrict__ oval, int32_t* __restrict__ perm) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) perm[i] = (int32_t)oval[i];
}

__global__ __launch_bounds__(256) void k_hv_gather(int64_t n, int64_t len, const int32_t* __restrict__ perm, const double* __restrict__ src,
                                                   double* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int32_t p = perm[i];
  dst[i] = (p >= 0 && p < len) ? src[p] : 0.0;
}

__global__ __launch_bounds__(256) void k_hv_fill(int64_t n, double v, double* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = v;
}

__global__ __launch_bounds__(256) void k_hv_sorted(int64_t n, const double* __restrict__ xs, uint32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double v = xs[i];
  if (!(v == v) || (i > 0 && !(xs[i - 1] <= v))) atomicOr(status, HV_ST_ORDER);
}

// One wave per evaluation point (four to a workgroup).  Every search is bounded by [0, n]: a list that is not ascending gives
// a wrong window, never a read outside it.
__global__ __launch_bounds__(256) void k_hv_locfit(int64_t n, const double* __restrict__ xs, const double* __restrict__ ys, const double* __restrict__ w,
                                                   int64_t k, int64_t m, const double* __restrict__ at, double* __restrict__ fit,
                                                   double* __restrict__ hout) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int64_t e = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (e >= m) return;                                      // the whole wave
  const double x = at[e];
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  if (!isfinite(x)) {
    if (lane == 0) { fit[e] = nan; if (hout) hout[e] = nan; }
    return;
  }
  // the k nearest are xs[l .. l + k): the smallest l whose left end is no farther than the point behind its right end
  int64_t lo = 0, hi = n - k;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (x - xs[mid] > xs[mid + k] - x) lo = mid + 1; else hi = mid;
  }
  const double h = fmax(fabs(xs[lo] - x), fabs(xs[lo + k - 1] - x));
  // the window |xs_i - x| <= h: [i0, i1)
  int64_t i0, i1;
  {
    int64_t a = 0, b = n;
    while (a < b) {
      const int64_t mid = (a + b) >> 1;
      if (x - xs[mid] > h) a = mid + 1; else b = mid;
    }
    i0 = a;
    b = n;
    while (a < b) {
      const int64_t mid = (a + b) >> 1;
      if (xs[mid] - x <= h) a = mid + 1; else b = mid;
    }
    i1 = a;
  }
  double S0 = 0.0, S1 = 0.0, S2 = 0.0, S3 = 0.0, S4 = 0.0, T0 = 0.0, T1 = 0.0, T2 = 0.0;
  for (int64_t i = i0 + lane; i < i1; i += 64) {
    double u = 0.0, W = 1.0;
    if (h > 0.0) {
      u = (xs[i] - x) / h;
      const double au = fabs(u);
      if (au < 1.0) {
        const double c = 1.0 - au * au * au;
        W = c * c * c;
      } else {
        W = 0.0;
      }
    }
    const double ww = (w ? w[i] : 1.0) * W, y = ys[i];
    const double w1 = ww * u, w2 = w1 * u, w3 = w2 * u, w4 = w3 * u;
    S0 += ww; S1 += w1; S2 += w2; S3 += w3; S4 += w4;
    T0 += ww * y; T1 += w1 * y; T2 += w2 * y;
  }
  S0 = gficf_wave_sum(S0); S1 = gficf_wave_sum(S1); S2 = gficf_wave_sum(S2); S3 = gficf_wave_sum(S3); S4 = gficf_wave_sum(S4);
  T0 = gficf_wave_sum(T0); T1 = gficf_wave_sum(T1); T2 = gficf_wave_sum(T2);
  if (lane != 0) return;
  if (hout) hout[e] = h;
  double b0 = nan;
  if (S0 > 0.0) {
    const double tol = 1e-10 * S0;
    const double l1 = S1 / S0, l2 = S2 / S0;
    const double p1 = S2 - l1 * S1, a12 = S3 - l1 * S2, a22 = S4 - l2 * S2, r1 = T1 - l1 * T0, r2 = T2 - l2 * T0;
    if (!(h > 0.0) || p1 < tol) {
      b0 = T0 / S0;
    } else {
      const double mm = a12 / p1, p2 = a22 - mm * a12;
      if (p2 < tol) {
        const double b1 = r1 / p1;
        b0 = (T0 - S1 * b1) / S0;
      } else {
        const double b2 = (r2 - mm * r1) / p2, b1 = (r1 - a12 * b2) / p1;
        b0 = (T0 - S1 * b1 - S2 * b2) / S0;
      }
    }
  }
  fit[e] = b0;
}

__global__ __launch_bounds__(256) void k_hv_res(int64_t n, const double* __restrict__ ys, const double* __restrict__ fit, double* __restrict__ res,
                                                double* __restrict__ ares) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double r = ys[i] - fit[i];
  res[i] = r;
  ares[i] = fabs(r);
}

// R's median of the ascending v[0 .. n)
__global__ void k_hv_median(int64_t n, const double* __restrict__ v, double* __restrict__ out) {
#pragma clang fp contract(off)
  if (blockIdx.x == 0 && threadIdx.x == 0) out[0] = (n & 1) ? v[n / 2] : (v[n / 2 - 1] + v[n / 2]) / 2.0;
}

__global__ __launch_bounds__(256) void k_hv_bisquare(int64_t n, const double* __restrict__ res, const double* __restrict__ s_at, double* __restrict__ w) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double s = s_at[0];
  if (!(s > 0.0)) return;                                  // the weights stay: every later fit is this one
  const double r = res[i] / (6.0 * s);
  double t = 1.0 - r * r;
  if (!(t > 0.0)) t = 0.0;
  w[i] = t * t;
}

__global__ __launch_bounds__(256) void k_hv_gap(int64_t n, const double* __restrict__ xs, double x0, double step, double half, int64_t len,
                                                double* __restrict__ grid, int32_t* __restrict__ gap) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= len) return;
  const double g = x0 + (double)i * step;
  grid[i] = g;
  gap[i] = (int32_t)(gficf_lower_bound(xs, n, g + half) - gficf_lower_bound(xs, n, g - half));
}

__global__ __launch_bounds__(256) void k_hv_curve(int64_t len, double x0, double b, double a, double* __restrict__ g1, double* __restrict__ yf) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= len) return;
  const double g = x0 + (double)i * 0.001;
  g1[i] = g;
  yf[i] = 0.5 * log10(b / pow(10.0, g) + a);
}

// One wave per gene.
__global__ __launch_bounds__(256) void k_hv_dist(int64_t n, const double* __restrict__ lx, const double* __restrict__ ly, int64_t len,
                                                 const double* __restrict__ g1, const double* __restrict__ yf, double* __restrict__ cvdist,
                                                 int32_t* __restrict__ index) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int64_t e = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (e >= n) return;                                      // the whole wave
  const double x = lx[e], y = ly[e];
  const int64_t j0 = gficf_lower_bound(g1, len, x - 0.2), j1 = gficf_lower_bound(g1, len, x + 0.2);
  double best = __longlong_as_double(0x7ff0000000000000ll);
  int64_t bi = -1;
  for (int64_t j = j0 + lane; j < j1; j += 64) {
    const double dx = g1[j] - x, dy = yf[j] - y;
    const double d = sqrt(dx * dx + dy * dy);
    if (d < best) { best = d; bi = j; }                    // a NaN is passed over, as which.min does
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double ob = __shfl_xor(best, d);
    const long long oi = __shfl_xor((long long)bi, d);
    if (oi >= 0 && (bi < 0 || ob < best || (ob == best && oi < bi))) { best = ob; bi = oi; }
  }
  if (lane != 0) return;
  double out = __longlong_as_double(0x7ff8000000000000ll);
  if (bi >= 0) {
    const double sd = (g1[bi] > x) ? -best : (yf[bi] < y ? best : -best);
    out = log2(pow(10.0, sd));
  }
  cvdist[e] = out;
  if (index) index[e] = (int32_t)bi;
}

// One workgroup.  v: the values as they lie; sv: the same ascending.  stats: bw, (distMid), lo, hi, sd, q1, q3, mean
__global__ __launch_bounds__(256) void k_hv_kde_stats(int64_t n, const double* __restrict__ v, const double* __restrict__ sv, double* __restrict__ stats) {
#pragma clang fp contract(off)
  __shared__ double s_fold[256];
  const int t = threadIdx.x;
  double a = 0.0;
  for (int64_t i = t; i < n; i += 256) a += v[i];
  const double mean = gficf_block_sum_f64(a, s_fold) / (double)n;
  double b = 0.0;
  for (int64_t i = t; i < n; i += 256) { const double d = v[i] - mean; b += d * d; }
  const double sd = sqrt(gficf_block_sum_f64(b, s_fold) / (double)(n - 1));
  if (t != 0) return;
  double q[2];
  for (int j = 0; j < 2; ++j) {
    const double idx = (double)(n - 1) * (j == 0 ? 0.25 : 0.75), lo = floor(idx), hi = ceil(idx), h = idx - lo;
    double r = sv[(int64_t)lo];
    const double xh = sv[(int64_t)hi];
    if (idx > lo && xh != r) r = (1.0 - h) * r + h * xh;
    q[j] = r;
  }
  double lo = fmin(sd, (q[1] - q[0]) / 1.34);
  if (lo == 0.0) lo = sd;
  if (lo == 0.0) lo = fabs(sv[0]);                          // sd = 0: every value is x_1
  if (lo == 0.0) lo = 1.0;
  const double bw = 0.9 * lo * pow((double)n, -0.2);
  stats[0] = bw;
  stats[2] = sv[0] - 3.0 * bw;
  stats[3] = sv[n - 1] + 3.0 * bw;
  stats[4] = sd;
  stats[5] = q[0];
  stats[6] = q[1];
  stats[7] = mean;
}

__device__ inline double hv_kde_grid(const double* stats, int j) {
#pragma clang fp contract(off)
  const double lo = stats[2], hi = stats[3];
  return j == GFICF_HVG_KDE_N - 1 ? hi : lo + (double)j * ((hi - lo) / (double)(GFICF_HVG_KDE_N - 1));
}

// One workgroup per grid point.
__global__ __launch_bounds__(256) void k_hv_kde_dens(int64_t n, const double* __restrict__ v, const double* __restrict__ stats, double* __restrict__ dens) {
#pragma clang fp contract(off)
  __shared__ double s_fold[256];
  const int t = threadIdx.x;
  const double g = hv_kde_grid(stats, (int)blockIdx.x), bw = stats[0];
  double a = 0.0;
  for (int64_t i = t; i < n; i += 256) {
    const double z = (g - v[i]) / bw;
    a += exp(-0.5 * z * z);
  }
  const double d = gficf_block_sum_f64(a, s_fold);
  if (t == 0) dens[blockIdx.x] = d;
}

// One workgroup: the first maximum of the densities (a NaN never wins).
__global__ __launch_bounds__(256) void k_hv_kde_mode(const double* __restrict__ dens, double* __restrict__ stats, int32_t* __restrict__ argmax) {
  __shared__ double s_v[256];
  __shared__ int s_i[256];
  const int t = threadIdx.x;
  double bv = dens[t];
  int bi = t;
  for (int j = t + 256; j < GFICF_HVG_KDE_N; j += 256)
    if (dens[j] > bv || !(bv == bv)) { bv = dens[j]; bi = j; }
  s_v[t] = bv;
  s_i[t] = bi;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (t < h) {
      const double ov = s_v[t + h];
      const int oi = s_i[t + h];
      const double mv = s_v[t];
      if (ov > mv || !(mv == mv) || (ov == mv && oi < s_i[t])) { s_v[t] = ov; s_i[t] = oi; }
    }
    __syncthreads();
  }
  if (t == 0) {
    argmax[0] = s_i[0];
    stats[1] = hv_kde_grid(stats, s_i[0]);
  }
}

// ------------------------------------------------------- workspace
struct HvWs {
  uint32_t* status;
  int32_t* count;
  size_t tr_bytes;
  char* tr_ws;
  int64_t* tptr;
  int32_t* tidx;
  double* tx;
  gficf_sort_bufs sort;
  int32_t *perm, *perm2;
  double *xs, *ys, *w, *fit, *res, *ares, *srt, *cv, *s;
  double *g5, *yseq, *g1, *yf;
  int32_t *gap, *argmax;
  double *kstats, *dens;
};

static size_t hv_carve(char* base, int64_t G, int64_t N, int64_t nnz, int64_t grid, HvWs& w) {
  gficf_carver cv;
  cv.base = base;
  const size_t g1 = (size_t)(G > 0 ? G : 1), n1 = (size_t)(nnz > 0 ? nnz : 1), gr = (size_t)(grid > 0 ? grid : 1);
  w.status = cv.take<uint32_t>(1);
  w.count = cv.take<int32_t>(1);
  w.tr_bytes = N > 0 ? gficf_csc_transpose_workspace_bytes(G, N) : 0;
  w.tr_ws = cv.take<char>(w.tr_bytes);
  w.tptr = cv.take<int64_t>(N > 0 ? g1 + 1 : 1);
  w.tidx = cv.take<int32_t>(N > 0 ? n1 : 1);
  w.tx = cv.take<double>(N > 0 ? n1 : 1);
  w.sort.take(cv, g1, g1, {});
  w.perm = cv.take<int32_t>(g1);
  w.perm2 = cv.take<int32_t>(g1);
  w.xs = cv.take<double>(g1);
  w.ys = cv.take<double>(g1);
  w.w = cv.take<double>(g1);
  w.fit = cv.take<double>(g1);
  w.res = cv.take<double>(g1);
  w.ares = cv.take<double>(g1);
  w.srt = cv.take<double>(g1);
  w.cv = cv.take<double>(g1);
  w.s = cv.take<double>(8);
  w.g5 = cv.take<double>(gr);
  w.yseq = cv.take<double>(gr);
  w.g1 = cv.take<double>(gr);
  w.yf = cv.take<double>(gr);
  w.gap = cv.take<int32_t>(gr);
  w.argmax = cv.take<int32_t>(1);
  w.kstats = cv.take<double>(8);
  w.dens = cv.take<double>(GFICF_HVG_KDE_N);
  return cv.total();
}

static unsigned hv_grid(int64_t n) { return (unsigned)gficf_ceil_div(n > 0 ? n : 1, 256); }
static unsigned hv_waves(int64_t n) { return (unsigned)gficf_ceil_div(n > 0 ? n : 1, 4); }

static bool hv_sizes_ok(int64_t G, int64_t N, int64_t nnz, int64_t grid) {
  return G >= 1 && G <= (int64_t)INT32_MAX / 64 && N >= 0 && N <= INT32_MAX && nnz >= 0 && nnz <= (int64_t)UINT32_MAX - 1 && grid >= 0 &&
         grid <= GFICF_HVG_GRID1_MAX;
}

// the workspace for lists of n values and grids of `grid` points carved from the caller's block
static int hv_workspace(void* ws, size_t ws_bytes, int64_t n, int64_t N, int64_t nnz, int64_t grid, HvWs& w) {
  if (!ws) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL workspace");
  if (!hv_sizes_ok(n, N, nnz, grid)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "n = %lld, N = %lld, nnz = %lld, grid = %lld: a size is out of range", (long long)n, (long long)N, (long long)nnz, (long long)grid);
  return gficf_addon_carve(ws, ws_bytes, [&](char* base) { return hv_carve(base, n, N, nnz, grid, w); });
}

// w.sort.oval = the stable ascending order of v[0 .. n) (the invalid last), *count = how many are valid
static int hv_order(gficf_ctx* ctx, const HvWs& w, int64_t n, const double* d_v, const int32_t* d_valid, int32_t* d_count) {
  GFICF_HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(int32_t), ctx->stream));
  return gficf_sort_f64(ctx, w.sort, n, {d_v, 0, d_valid, nullptr, 0u, d_count, nullptr, 0u, 0});
}

// dst = v ascending (n values, all valid); uses w.perm2
static int hv_sorted_copy(gficf_ctx* ctx, const HvWs& w, int64_t n, const double* d_v, double* d_dst) {
  int rc = hv_order(ctx, w, n, d_v, nullptr, w.count);
  if (rc) return rc;
  hipLaunchKernelGGL(k_hv_perm, dim3(hv_grid(n)), dim3(256), 0, ctx->stream, n, (const uint32_t*)w.sort.oval, w.perm2);
  hipLaunchKernelGGL(k_hv_gather, dim3(hv_grid(n)), dim3(256), 0, ctx->stream, n, n, (const int32_t*)w.perm2, d_v, d_dst);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

static int hv_locfit(gficf_ctx* ctx, int64_t n, const double* d_xs, const double* d_ys, const double* d_w, int64_t k, int64_t m, const double* d_at,
                     double* d_fit, double* d_h) {
  if (m == 0) return GFICF_OK;
  hipLaunchKernelGGL(k_hv_locfit, dim3(hv_waves(m)), dim3(256), 0, ctx->stream, n, d_xs, d_ys, d_w, k, m, d_at, d_fit, d_h);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

static int hv_robust(gficf_ctx* ctx, const HvWs& w, int64_t n, const double* d_xs, const double* d_ys, const double* d_w_in, int64_t k, int iters,
                     double* d_w, double* d_fit, double* d_s) {
  hipStream_t st = ctx->stream;
  if (d_w_in) {
    if (d_w_in != d_w) GFICF_HIP_CHECK(hipMemcpyAsync(d_w, d_w_in, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
  } else {
    hipLaunchKernelGGL(k_hv_fill, dim3(hv_grid(n)), dim3(256), 0, st, n, 1.0, d_w);
  }
  for (int it = 0;; ++it) {
    int rc = hv_locfit(ctx, n, d_xs, d_ys, d_w, k, n, d_xs, d_fit, nullptr);
    if (rc) return rc;
    if (it == iters) break;
    hipLaunchKernelGGL(k_hv_res, dim3(hv_grid(n)), dim3(256), 0, st, n, d_ys, (const double*)d_fit, w.res, w.ares);
    GFICF_HIP_CHECK(hipGetLastError());
    rc = hv_sorted_copy(ctx, w, n, w.ares, w.srt);
    if (rc) return rc;
    hipLaunchKernelGGL(k_hv_median, dim3(1), dim3(64), 0, st, n, (const double*)w.srt, d_s + it);
    hipLaunchKernelGGL(k_hv_bisquare, dim3(hv_grid(n)), dim3(256), 0, st, n, (const double*)w.res, (const double*)(d_s + it), d_w);
    GFICF_HIP_CHECK(hipGetLastError());
  }
  return GFICF_OK;
}

static int hv_check_sorted(gficf_ctx* ctx, const HvWs& w, int64_t n, const double* d_xs) {
  GFICF_HIP_CHECK(hipMemsetAsync(w.status, 0, sizeof(uint32_t), ctx->stream));
  hipLaunchKernelGGL(k_hv_sorted, dim3(hv_grid(n)), dim3(256), 0, ctx->stream, n, d_xs, w.status);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

static int hv_curve_distance(gficf_ctx* ctx, const HvWs& w, int64_t n, const double* d_lx, const double* d_ly, double b, double a, double x0, int64_t len,
                             double* d_cvdist, int32_t* d_index) {
  hipLaunchKernelGGL(k_hv_curve, dim3(hv_grid(len)), dim3(256), 0, ctx->stream, len, x0, b, a, w.g1, w.yf);
  hipLaunchKernelGGL(k_hv_dist, dim3(hv_waves(n)), dim3(256), 0, ctx->stream, n, d_lx, d_ly, len, (const double*)w.g1, (const double*)w.yf, d_cvdist, d_index);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

static int hv_kde(gficf_ctx* ctx, const HvWs& w, int64_t n, const double* d_v, double* d_stats, double* d_dens, int32_t* d_argmax) {
  int rc = hv_sorted_copy(ctx, w, n, d_v, w.srt);
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(k_hv_kde_stats, dim3(1), dim3(256), 0, st, n, d_v, (const double*)w.srt, d_stats);
  hipLaunchKernelGGL(k_hv_kde_dens, dim3(GFICF_HVG_KDE_N), dim3(256), 0, st, n, d_v, (const double*)d_stats, d_dens);
  hipLaunchKernelGGL(k_hv_kde_mode, dim3(1), dim3(256), 0, st, (const double*)d_dens, d_stats, d_argmax);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

// R's length of seq(a, b, by)
static int64_t hv_seq_len(double a, double b, double by) { return (int64_t)std::floor((b - a) / by + 1e-10) + 1; }

// ------------------------------------------------------- the host decisions
// step 3: the 0-based indices first .. last of the grid points the curve is fitted through
static int hv_trusted(int64_t G, int64_t len, const double* g5, const int32_t* gap, const double* yseq, int64_t* cdx0, int64_t* j0) {
#pragma clang fp contract(off)
  *cdx0 = -1;
  const double need = 0.005 * (double)G;
  for (int64_t i = 0; i < len; ++i)
    if ((double)gap[i] > need) { *cdx0 = i; break; }
  *j0 = len - 2;
  for (int64_t j = 0; j + 1 < len; ++j)
    if (yseq[j + 1] - yseq[j] > 0.0 && g5[j + 1] > 0.0) { *j0 = j; break; }
  if (*cdx0 < 0 || *cdx0 > *j0 || *j0 - *cdx0 + 1 < 3 || *j0 + 1 >= len)
    GFICF_FAIL(GFICF_ERR_BAD_VALUE, "the variance-mean trend cannot be fitted: the trusted range holds %lld points (first dense window %lld, end %lld of %lld)",
               (long long)(*cdx0 < 0 || *cdx0 > *j0 ? 0 : *j0 - *cdx0 + 1), (long long)*cdx0, (long long)*j0, (long long)len);
  return GFICF_OK;
}

// |r|^2 of the model 0.5 * log10(b / x + a) at (b, a), or -1 where some b / x + a is not positive
static double hv_nls_dev(const std::vector<double>& x, const std::vector<double>& y, double b, double a, std::vector<double>* r, std::vector<double>* arg) {
#pragma clang fp contract(off)
  double dev = 0.0;
  for (size_t i = 0; i < x.size(); ++i) {
    const double t = b / x[i] + a;
    if (!(t > 0.0) || !std::isfinite(t)) return -1.0;
    const double ri = y[i] - 0.5 * std::log10(t);
    if (r) (*r)[i] = ri;
    if (arg) (*arg)[i] = t;
    dev += ri * ri;
  }
  return dev;
}

// step 4
static int hv_nls(const std::vector<double>& x, const std::vector<double>& y, double* b_out, double* a_out, int* rounds) {
#pragma clang fp contract(off)
  const size_t n = x.size();
  const double c = 0.5 / std::log(10.0);
  double b = 1.0, a = 0.0, fac = 1.0, yy = 0.0;
  for (size_t i = 0; i < n; ++i) yy += y[i] * y[i];
  std::vector<double> r(n), t(n), rn(n), tn(n), j1(n), j2(n);
  double dev = hv_nls_dev(x, y, b, a, &r, &t);
  if (dev < 0.0) GFICF_FAIL(GFICF_ERR_BAD_VALUE, "the variance-mean trend cannot be fitted: the curve is not defined at its start");
  for (int it = 0; it <= 500; ++it) {
    *rounds = it;
    // J = d model / d (b, a);  Q R = J by modified Gram-Schmidt;  q = Q^T r
    double n1 = 0.0;
    for (size_t i = 0; i < n; ++i) { j1[i] = c / (x[i] * t[i]); j2[i] = c / t[i]; n1 += j1[i] * j1[i]; }
    n1 = std::sqrt(n1);
    double r12 = 0.0;
    for (size_t i = 0; i < n; ++i) { j1[i] = j1[i] / n1; r12 += j1[i] * j2[i]; }
    double n2 = 0.0;
    for (size_t i = 0; i < n; ++i) { j2[i] = j2[i] - r12 * j1[i]; n2 += j2[i] * j2[i]; }
    n2 = std::sqrt(n2);
    double jn = 0.0;
    for (size_t i = 0; i < n; ++i) jn += (c / t[i]) * (c / t[i]);
    if (!(n1 > 0.0) || !(n2 > 1e-10 * std::sqrt(jn))) GFICF_FAIL(GFICF_ERR_BAD_VALUE, "the variance-mean trend cannot be fitted: singular gradient in round %d", it);
    double q1 = 0.0, q2 = 0.0;
    for (size_t i = 0; i < n; ++i) { j2[i] = j2[i] / n2; q1 += j1[i] * r[i]; q2 += j2[i] * r[i]; }
    const double qq = q1 * q1 + q2 * q2;
    if (dev <= 1e-26 * (yy + (double)n) || std::sqrt(qq / (dev - qq)) < 1e-5) {
      *b_out = b;
      *a_out = a;
      return GFICF_OK;
    }
    if (it == 500) break;
    const double da = q2 / n2, db = (q1 - r12 * da) / n1;
    for (;;) {
      if (fac < 1.0 / 1024.0) GFICF_FAIL(GFICF_ERR_BAD_VALUE, "the variance-mean trend cannot be fitted: step factor below 1/1024 in round %d", it);
      const double bn = b + fac * db, an = a + fac * da;
      const double dn = hv_nls_dev(x, y, bn, an, &rn, &tn);
      if (dn >= 0.0 && dn <= dev) {
        b = bn; a = an; dev = dn;
        r.swap(rn); t.swap(tn);
        fac = std::min(2.0 * fac, 1.0);
        break;
      }
      fac = fac / 2.0;
    }
  }
  GFICF_FAIL(GFICF_ERR_BAD_VALUE, "the variance-mean trend cannot be fitted: no convergence in 500 rounds");
}

// step 7 over the n valid genes
static void hv_pvalues(const std::vector<double>& cv, double mid, double* mu_out, double* sigma_out, std::vector<double>& P) {
#pragma clang fp contract(off)
  std::vector<double> tmp;
  tmp.reserve(2 * cv.size());
  for (double v : cv) { const double d = v - mid; if (d <= 0.0) tmp.push_back(d + mid); }
  for (double v : cv) { const double d = v - mid; if (d < 0.0) tmp.push_back(std::fabs(d) + mid); }
  double s = 0.0;
  for (double v : tmp) s += v;
  const double mu = s / (double)tmp.size();
  double q = 0.0;
  for (double v : tmp) q += (v - mu) * (v - mu);
  const double sigma = std::sqrt(q / (double)tmp.size());
  *mu_out = mu;
  *sigma_out = sigma;
  P.resize(cv.size());
  const double den = sigma * std::sqrt(2.0);
  for (size_t i = 0; i < cv.size(); ++i) P[i] = 0.5 * std::erfc((cv[i] - mu) / den);
}

struct HvOut {
  double *lx, *ly, *fit, *weights, *cvdist, *P, *scalars, *g5, *yseq;
  int32_t *valid, *gap;
};

// steps 2 - 7 from the device lists d_lx, d_ly, d_valid of G genes; the stream is idle at the return
static int hv_trend(gficf_ctx* ctx, gficf_host_io& io, const HvWs& w, int64_t G, const double* d_lx, const double* d_ly, const int32_t* d_valid,
                    const HvOut& o) {
  hipStream_t st = ctx->stream;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int i = 0; i < GFICF_HVG_SCALARS; ++i) o.scalars[i] = nan;
  int rc = hv_order(ctx, w, G, d_lx, d_valid, w.count);
  if (rc) return io.drain(rc);
  hipLaunchKernelGGL(k_hv_perm, dim3(hv_grid(G)), dim3(256), 0, st, G, (const uint32_t*)w.sort.oval, w.perm);
  int32_t n32 = 0;
  std::vector<int32_t> perm((size_t)G);
  io.down(&n32, w.count, sizeof(int32_t));
  io.down(perm.data(), w.perm, sizeof(int32_t) * (size_t)G);
  if (o.lx) io.down(o.lx, d_lx, sizeof(double) * (size_t)G);
  if (o.ly) io.down(o.ly, d_ly, sizeof(double) * (size_t)G);
  io.down(o.valid, d_valid, sizeof(int32_t) * (size_t)G);
  rc = io.finish(GFICF_OK);
  if (rc) return rc;
  const int64_t n = n32, k = (int64_t)std::floor(0.2 * (double)n);
  o.scalars[0] = (double)n;
  o.scalars[1] = (double)k;
  if (k < 4) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "%lld genes with a finite log10 mean and log10 cv: the local regression needs at least 20", (long long)n);
  hipLaunchKernelGGL(k_hv_gather, dim3(hv_grid(n)), dim3(256), 0, st, n, G, (const int32_t*)w.perm, d_lx, w.xs);
  hipLaunchKernelGGL(k_hv_gather, dim3(hv_grid(n)), dim3(256), 0, st, n, G, (const int32_t*)w.perm, d_ly, w.ys);
  rc = hv_robust(ctx, w, n, w.xs, w.ys, nullptr, k, 3, w.w, w.fit, w.s);
  if (rc) return io.drain(rc);
  double ends[2] = {0.0, 0.0};
  io.down(&ends[0], w.xs, sizeof(double));
  io.down(&ends[1], w.xs + (n - 1), sizeof(double));
  io.down(o.scalars + 2, w.s, 3 * sizeof(double));
  std::vector<double> fit((size_t)n), wt((size_t)n);
  io.down(fit.data(), w.fit, sizeof(double) * (size_t)n);
  io.down(wt.data(), w.w, sizeof(double) * (size_t)n);
  rc = io.finish(GFICF_OK);
  if (rc) return rc;
  for (int64_t g = 0; g < G; ++g) {
    if (o.fit) o.fit[g] = nan;
    if (o.weights) o.weights[g] = nan;
    if (o.cvdist) o.cvdist[g] = nan;
    o.P[g] = nan;
  }
  bool bad = false;
  for (int64_t i = 0; i < n; ++i) {
    const int32_t g = perm[(size_t)i];
    if (o.fit) o.fit[g] = fit[(size_t)i];
    if (o.weights) o.weights[g] = wt[(size_t)i];
    bad = bad || !std::isfinite(fit[(size_t)i]);
  }
  if (bad) GFICF_FAIL(GFICF_ERR_BAD_VALUE, "the local regression has no weight left at a gene");
  const int64_t len5 = hv_seq_len(ends[0], ends[1], 0.005), len1 = hv_seq_len(ends[0], ends[1], 0.001);
  o.scalars[5] = (double)len5;
  o.scalars[11] = (double)len1;
  if (len5 < 1 || len5 > GFICF_HVG_GRID5_MAX || len1 > GFICF_HVG_GRID1_MAX) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "a grid of %lld points", (long long)len1);
  hipLaunchKernelGGL(k_hv_gap, dim3(hv_grid(len5)), dim3(256), 0, st, n, (const double*)w.xs, ends[0], 0.005, 0.05, len5, w.g5, w.gap);
  rc = hv_locfit(ctx, n, w.xs, w.ys, w.w, k, len5, w.g5, w.yseq, nullptr);
  if (rc) return io.drain(rc);
  std::vector<double> g5((size_t)len5), yseq((size_t)len5);
  std::vector<int32_t> gap((size_t)len5);
  io.down(g5.data(), w.g5, sizeof(double) * (size_t)len5);
  io.down(yseq.data(), w.yseq, sizeof(double) * (size_t)len5);
  io.down(gap.data(), w.gap, sizeof(int32_t) * (size_t)len5);
  rc = io.finish(GFICF_OK);
  if (rc) return rc;
  if (o.g5) std::copy(g5.begin(), g5.end(), o.g5);
  if (o.yseq) std::copy(yseq.begin(), yseq.end(), o.yseq);
  if (o.gap) std::copy(gap.begin(), gap.end(), o.gap);
  for (int64_t i = 0; i < len5; ++i)
    if (!std::isfinite(yseq[(size_t)i])) GFICF_FAIL(GFICF_ERR_BAD_VALUE, "the local regression has no weight left at grid point %lld", (long long)i);
  int64_t cdx0 = -1, j0 = -1;
  rc = hv_trusted(G, len5, g5.data(), gap.data(), yseq.data(), &cdx0, &j0);
  o.scalars[6] = (double)cdx0;
  o.scalars[7] = (double)j0;
  if (rc) return rc;
  std::vector<double> px, py;
  for (int64_t i = cdx0 + 1; i <= j0 + 1; ++i) { px.push_back(std::pow(10.0, g5[(size_t)i])); py.push_back(yseq[(size_t)i]); }
  double b = 0.0, a = 0.0;
  int rounds = 0;
  rc = hv_nls(px, py, &b, &a, &rounds);
  if (rc) return rc;
  o.scalars[8] = b;
  o.scalars[9] = a;
  o.scalars[10] = (double)rounds;
  rc = hv_curve_distance(ctx, w, n, w.xs, w.ys, b, a, ends[0], len1, w.cv, nullptr);
  if (!rc) rc = hv_kde(ctx, w, n, w.cv, w.kstats, w.dens, w.argmax);
  if (rc) return io.drain(rc);
  std::vector<double> cvd((size_t)n), P;
  double ks[8];
  io.down(cvd.data(), w.cv, sizeof(double) * (size_t)n);
  io.down(ks, w.kstats, sizeof(ks));
  rc = io.finish(GFICF_OK);
  if (rc) return rc;
  o.scalars[12] = ks[0];
  o.scalars[13] = ks[1];
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(cvd[(size_t)i])) GFICF_FAIL(GFICF_ERR_BAD_VALUE, "the variance-mean trend cannot be fitted: the curve is not defined near a gene");
  hv_pvalues(cvd, ks[1], &o.scalars[14], &o.scalars[15], P);
  for (int64_t i = 0; i < n; ++i) {
    const int32_t g = perm[(size_t)i];
    if (o.cvdist) o.cvdist[g] = cvd[(size_t)i];
    o.P[g] = P[(size_t)i];
  }
  return GFICF_OK;
}

}  // namespace

extern "C" {

int gficf_hvg_abi_version(void) { return GFICF_HVG_ABI_VERSION; }

size_t gficf_hvg_workspace_bytes(int64_t G, int64_t N, int64_t nnz, int64_t grid_pts) {
  if (!hv_sizes_ok(G, N, nnz, grid_pts)) return 0;
  HvWs w;
  return hv_carve(nullptr, G, N, nnz, grid_pts, w);
}

int gficf_hvg_moments_device(gficf_ctx* ctx, int64_t G, int64_t N, const int64_t* d_colptr, const int32_t* d_rowidx, const double* d_x, int64_t nnz,
                             void* ws, size_t ws_bytes, double* d_mean, double* d_sd, double* d_var, int32_t* d_nobs, double* d_lx, double* d_ly,
                             int32_t* d_valid) {
  GFICF_CTX_ENTER(ctx);
  if (N < 2) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "N = %lld: the standard deviation needs at least 2 cells", (long long)N);
  if (!d_colptr || !d_mean || !d_sd || !d_var || !d_nobs || !d_lx || !d_ly || !d_valid || (nnz > 0 && (!d_rowidx || !d_x)))
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  HvWs w;
  int rc = hv_workspace(ws, ws_bytes, G, N, nnz, 0, w);
  if (rc) return rc;
  GFICF_HIP_CHECK(hipMemsetAsync(w.status, 0, sizeof(uint32_t), ctx->stream));
  rc = gficf_csc_transpose_device(ctx, G, N, d_colptr, d_rowidx, d_x, nnz, w.tptr, w.tidx, w.tx, w.tr_ws, w.tr_bytes);
  if (rc) return rc;
  hipLaunchKernelGGL(k_hv_moments, dim3(hv_waves(G)), dim3(256), 0, ctx->stream, G, N, nnz, (const int64_t*)w.tptr, (const double*)w.tx, d_mean, d_sd, d_var,
                     d_nobs, d_lx, d_ly, d_valid);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int gficf_hvg_order_device(gficf_ctx* ctx, int64_t n, const double* d_key, const int32_t* d_valid, void* ws, size_t ws_bytes, int32_t* d_perm,
                           int32_t* d_count) {
  GFICF_CTX_ENTER(ctx);
  if (!d_key || !d_perm || !d_count) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  HvWs w;
  int rc = hv_workspace(ws, ws_bytes, n, 0, 0, 0, w);
  if (rc) return rc;
  rc = hv_order(ctx, w, n, d_key, d_valid, d_count);
  if (rc) return rc;
  hipLaunchKernelGGL(k_hv_perm, dim3(hv_grid(n)), dim3(256), 0, ctx->stream, n, (const uint32_t*)w.sort.oval, d_perm);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int gficf_hvg_locfit_device(gficf_ctx* ctx, int64_t n, const double* d_xs, const double* d_ys, const double* d_w, int64_t k, int64_t m,
                            const double* d_at, void* ws, size_t ws_bytes, double* d_fit, double* d_h) {
  GFICF_CTX_ENTER(ctx);
  if (k < 1 || k > n || m < 0 || m > (int64_t)INT32_MAX / 64) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "k = %lld of n = %lld points, m = %lld: out of range", (long long)k, (long long)n, (long long)m);
  if (!d_xs || !d_ys || (m > 0 && (!d_at || !d_fit))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  HvWs w;
  int rc = hv_workspace(ws, ws_bytes, n, 0, 0, 0, w);
  if (rc) return rc;
  rc = hv_check_sorted(ctx, w, n, d_xs);
  if (rc) return rc;
  return hv_locfit(ctx, n, d_xs, d_ys, d_w, k, m, d_at, d_fit, d_h);
}

int gficf_hvg_robust_device(gficf_ctx* ctx, int64_t n, const double* d_xs, const double* d_ys, const double* d_w_in, int64_t k, int32_t iters,
                            void* ws, size_t ws_bytes, double* d_w, double* d_fit, double* d_s) {
  GFICF_CTX_ENTER(ctx);
  if (k < 1 || k > n || iters < 0 || iters > 64) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "k = %lld of n = %lld points, iters = %d: out of range", (long long)k, (long long)n, iters);
  if (!d_xs || !d_ys || !d_w || !d_fit || (iters > 0 && !d_s)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  HvWs w;
  int rc = hv_workspace(ws, ws_bytes, n, 0, 0, 0, w);
  if (rc) return rc;
  rc = hv_check_sorted(ctx, w, n, d_xs);
  if (rc) return rc;
  return hv_robust(ctx, w, n, d_xs, d_ys, d_w_in, k, iters, d_w, d_fit, d_s);
}

int gficf_hvg_gap_device(gficf_ctx* ctx, int64_t n, const double* d_xs, double x0, double step, double half, int64_t len, void* ws, size_t ws_bytes,
                         double* d_grid, int32_t* d_gap) {
  GFICF_CTX_ENTER(ctx);
  if (len < 1 || len > GFICF_HVG_GRID1_MAX) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "a grid of %lld points", (long long)len);
  if (!d_xs || !d_grid || !d_gap) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  HvWs w;
  int rc = hv_workspace(ws, ws_bytes, n, 0, 0, 0, w);
  if (rc) return rc;
  rc = hv_check_sorted(ctx, w, n, d_xs);
  if (rc) return rc;
  hipLaunchKernelGGL(k_hv_gap, dim3(hv_grid(len)), dim3(256), 0, ctx->stream, n, d_xs, x0, step, half, len, d_grid, d_gap);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int gficf_hvg_curve_distance_device(gficf_ctx* ctx, int64_t n, const double* d_lx, const double* d_ly, double b, double a, double x0, int64_t len,
                                    void* ws, size_t ws_bytes, double* d_cvdist, int32_t* d_index) {
  GFICF_CTX_ENTER(ctx);
  if (len < 1) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "a grid of %lld points", (long long)len);
  if (!d_lx || !d_ly || !d_cvdist) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  HvWs w;
  int rc = hv_workspace(ws, ws_bytes, n, 0, 0, len, w);
  if (rc) return rc;
  GFICF_HIP_CHECK(hipMemsetAsync(w.status, 0, sizeof(uint32_t), ctx->stream));
  return hv_curve_distance(ctx, w, n, d_lx, d_ly, b, a, x0, len, d_cvdist, d_index);
}

int gficf_hvg_kde_device(gficf_ctx* ctx, int64_t n, const double* d_v, void* ws, size_t ws_bytes, double* d_stats, double* d_dens, int32_t* d_argmax) {
  GFICF_CTX_ENTER(ctx);
  if (n < 2) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "n = %lld: the bandwidth needs at least 2 values", (long long)n);
  if (!d_v || !d_stats || !d_dens || !d_argmax) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  HvWs w;
  int rc = hv_workspace(ws, ws_bytes, n, 0, 0, 0, w);
  if (rc) return rc;
  GFICF_HIP_CHECK(hipMemsetAsync(w.status, 0, sizeof(uint32_t), ctx->stream));
  return hv_kde(ctx, w, n, d_v, d_stats, d_dens, d_argmax);
}

int gficf_hvg_sync(gficf_ctx* ctx, const void* ws) {
  uint32_t st;
  const int rc = gficf_addon_read_status(ctx, ws, &st);
  if (rc) return rc;
  if (st & HV_ST_ORDER) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "the points of the local fit are not in ascending order (or hold a NaN)");
  return GFICF_OK;
}

int gficf_hvg_trend_host(gficf_ctx* ctx, int64_t G, const double* mean, const double* cv, double* lx, double* ly, int32_t* valid, double* fit,
                         double* weights, double* cvdist, double* P, double* scalars, double* g5, int32_t* gap, double* yseq) {
  GFICF_CTX_ENTER(ctx);
  if (!hv_sizes_ok(G, 0, 0, 0)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "G = %lld: out of range", (long long)G);
  if (!mean || !cv || !valid || !P || !scalars) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  const size_t wsb = gficf_hvg_workspace_bytes(G, 0, 0, GFICF_HVG_GRID1_MAX);
  gficf_host_io io{ctx, "gficf_hvg_trend_host"};
  gficf_carver cv_;
  double *d_mean, *d_cv, *d_lx, *d_ly; int32_t* d_valid; char* d_ws;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    d_mean = cv_.take<double>((size_t)G); d_cv = cv_.take<double>((size_t)G); d_lx = cv_.take<double>((size_t)G); d_ly = cv_.take<double>((size_t)G);
    d_valid = cv_.take<int32_t>((size_t)G); d_ws = cv_.take<char>(wsb);
    if (pass == 0) io.e = cv_.bind(ctx, GFICF_SLOT_STAGE0);
  }
  io.up(d_mean, mean, sizeof(double) * (size_t)G);
  io.up(d_cv, cv, sizeof(double) * (size_t)G);
  if (!io.ok()) return io.drain(GFICF_OK);
  HvWs w;
  int rc = hv_workspace(d_ws, wsb, G, 0, 0, GFICF_HVG_GRID1_MAX, w);
  if (rc) return io.drain(rc);
  hipLaunchKernelGGL(k_hv_logs, dim3(hv_grid(G)), dim3(256), 0, ctx->stream, G, (const double*)d_mean, (const double*)d_cv, d_lx, d_ly, d_valid);
  const HvOut o{lx, ly, fit, weights, cvdist, P, scalars, g5, yseq, valid, gap};
  return hv_trend(ctx, io, w, G, d_lx, d_ly, d_valid, o);
}

int gficf_hvg_host(gficf_ctx* ctx, int64_t G, int64_t N, const void* colptr, int colptr_is_i64, const int32_t* rowidx, const double* x,
                   int32_t only_moments, double* mean, double* sd, double* var, int32_t* nobs, double* lx, double* ly, int32_t* valid, double* fit,
                   double* weights, double* cvdist, double* P, double* scalars, double* g5, int32_t* gap, double* yseq) {
  GFICF_CTX_ENTER(ctx);
  if (G < 1 || N < 2) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "G = %lld, N = %lld: at least one gene and two cells", (long long)G, (long long)N);
  if (!colptr || !valid || (!only_moments && (!P || !scalars))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  std::vector<int64_t> cp;
  int64_t nnz = 0;
  int rc = gficf_host_colptr(colptr, colptr_is_i64, N, "colptr", cp, &nnz);
  if (rc) return rc;
  if (!hv_sizes_ok(G, N, nnz, 0)) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "G = %lld, N = %lld, nnz = %lld: beyond what the sort and the transpose take", (long long)G, (long long)N, (long long)nnz);
  if (nnz > 0 && (!rowidx || !x)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  const int64_t grid = only_moments ? 0 : GFICF_HVG_GRID1_MAX;
  const size_t ne = (size_t)(nnz > 0 ? nnz : 1), wsb = gficf_hvg_workspace_bytes(G, N, nnz, grid);
  gficf_host_io io{ctx, "gficf_hvg_host"};
  gficf_carver cv;
  int64_t* d_cp; int32_t *d_row, *d_nobs, *d_valid; double *d_x, *d_mean, *d_sd, *d_var, *d_lx, *d_ly; char* d_ws;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    d_cp = cv.take<int64_t>((size_t)N + 1); d_row = cv.take<int32_t>(ne); d_x = cv.take<double>(ne);
    d_mean = cv.take<double>((size_t)G); d_sd = cv.take<double>((size_t)G); d_var = cv.take<double>((size_t)G); d_lx = cv.take<double>((size_t)G);
    d_ly = cv.take<double>((size_t)G); d_nobs = cv.take<int32_t>((size_t)G); d_valid = cv.take<int32_t>((size_t)G); d_ws = cv.take<char>(wsb);
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_STAGE0);
  }
  io.up(d_cp, cp.data(), sizeof(int64_t) * ((size_t)N + 1));
  io.up(d_row, rowidx, sizeof(int32_t) * (size_t)nnz);
  io.up(d_x, x, sizeof(double) * (size_t)nnz);
  if (!io.ok()) return io.drain(GFICF_OK);
  rc = gficf_hvg_moments_device(ctx, G, N, d_cp, d_row, d_x, nnz, d_ws, wsb, d_mean, d_sd, d_var, d_nobs, d_lx, d_ly, d_valid);
  if (rc) return io.drain(rc);
  if (mean) io.down(mean, d_mean, sizeof(double) * (size_t)G);
  if (sd) io.down(sd, d_sd, sizeof(double) * (size_t)G);
  if (var) io.down(var, d_var, sizeof(double) * (size_t)G);
  if (nobs) io.down(nobs, d_nobs, sizeof(int32_t) * (size_t)G);
  if (only_moments) {
    if (lx) io.down(lx, d_lx, sizeof(double) * (size_t)G);
    if (ly) io.down(ly, d_ly, sizeof(double) * (size_t)G);
    io.down(valid, d_valid, sizeof(int32_t) * (size_t)G);
  }
  if (!io.ok()) return io.drain(GFICF_OK);
  rc = gficf_hvg_sync(ctx, d_ws);                          // the moments are on the host, the input is checked
  if (rc || only_moments) return rc;
  HvWs w;
  rc = hv_workspace(d_ws, wsb, G, N, nnz, grid, w);
  if (rc) return rc;
  const HvOut o{lx, ly, fit, weights, cvdist, P, scalars, g5, yseq, valid, gap};
  return hv_trend(ctx, io, w, G, d_lx, d_ly, d_valid, o);
}

}  // extern "C"
