// od.hip — the overdispersed genes of findOverDispersed() (reference R/dimensinalityReduction.R:235-308, after pagoda2): the
// penalised cubic regression spline of every gene's log variance on its ICF weight, the F-test log p-value of its residual and
// the BH adjustment in log space, the chi-square adjusted variance and the gene scale factor; and the pass that selects and
// scales rows of the GF-ICF matrix for runPCA / runLSA / embedNewCells.  Built into libgficf_od.so, which links libgficf_hip.so
// (context, pool, radix sort, error plumbing) and libgficf_hvg.so (gficf_hvg_moments_device); include/gficf_od.h states the contract.
//
// Launches, all on the context's stream:
//   k_od_valid        v = log(var), the valid flags
//   (addon_sort.h: k_sort_keys, k_sort_next<0>, radix sort x 2)   the stable order of the valid m
//   k_od_knots        one workgroup: the distinct sorted m by a chunked scan, the knots, F = B^-1 D
//   k_od_sum_v, k_od_fold      the sum of the valid v: partial folded sums, then their fold
//   k_od_sums, k_od_fold       X^T X, X^T (v - vbar), sum (v - vbar)^2 the same way
//   (host)            Cholesky, the penalty's eigenvalues, the GCV search, beta
//   k_od_fit          fit and res per gene
//   k_od_scores       one thread per gene: lp (continued fraction), qv (Newton in log space), gsf
//   k_od_logpf, k_od_logqchisq   the two special functions over arrays
//   (sort), k_od_bh   one workgroup: q in sorted order, the running minimum from the end by chunks, the scatter
//   k_od_newid        one workgroup: the new row numbers of the selected rows (chunked scan)
//   k_od_count, k_od_colscan, k_od_write   one wave per column: kept entries; the new column pointers; the compacted, scaled columns
//   k_od_scale        values only (no mask)
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "addon_sort.h"
#include "addon_status.h"
#include "common.h"
#include "gficf_hvg.h"
#include "gficf_od.h"

namespace {

constexpr uint32_t OD_ST_ITER = 1u;                        // an iteration of a special function hit its cap
constexpr uint32_t OD_ST_CSC = 2u;                         // a row index or a column pointer of the matrix out of range
constexpr int KM = GFICF_OD_K_MAX;
constexpr int OD_NS = 1 + KM * (KM + 1) / 2 + KM;          // sum (v - vbar)^2, X^T X (upper triangle by rows), X^T (v - vbar)
constexpr int OD_BASIS = 3 + KM + KM * KM;                 // n, u, kk, the knots, F (row stride KM)
constexpr int OD_CF_CAP = 200000;                          // terms of a continued fraction or a series
constexpr int OD_NEWTON_CAP = 200;

// F = B^-1 D padded with a zero first and last row (row stride KM) for the kk knots kn[]; kk < 3: all zero
__host__ __device__ inline void od_basis_F(int kk, const double* kn, double* F) {
#pragma clang fp contract(off)
  for (int i = 0; i < KM * KM; ++i) F[i] = 0.0;
  if (kk < 3) return;
  double h[KM], dg[KM], up[KM];
  const int q = kk - 2;
  for (int j = 0; j + 1 < kk; ++j) h[j] = kn[j + 1] - kn[j];
  // B: diagonal (h_i + h_{i+1}) / 3, off-diagonal h_{i+1} / 6; Thomas elimination, then every column of D
  for (int i = 0; i < q; ++i) { dg[i] = (h[i] + h[i + 1]) / 3.0; up[i] = h[i + 1] / 6.0; }
  double cp[KM];
  cp[0] = up[0] / dg[0];
  for (int i = 1; i < q; ++i) { dg[i] = dg[i] - up[i - 1] * cp[i - 1]; cp[i] = up[i] / dg[i]; }
  for (int c = 0; c < kk; ++c) {
    double y[KM];
    for (int i = 0; i < q; ++i) {
      double d = 0.0;
      if (c == i) d = 1.0 / h[i];
      else if (c == i + 1) d = -1.0 / h[i] - 1.0 / h[i + 1];
      else if (c == i + 2) d = 1.0 / h[i + 1];
      y[i] = i == 0 ? d / dg[0] : (d - up[i - 1] * y[i - 1]) / dg[i];
    }
    for (int i = q - 2; i >= 0; --i) y[i] = y[i] - cp[i] * y[i + 1];
    for (int i = 0; i < q; ++i) F[(i + 1) * KM + c] = y[i];
  }
}

// the design row of m (entries kk .. KM - 1 are zero)
__host__ __device__ inline void od_row(int kk, const double* kn, const double* F, double m, double* row) {
#pragma clang fp contract(off)
  for (int i = 0; i < KM; ++i) row[i] = 0.0;
  if (kk < 2) { row[0] = 1.0; return; }
  int j = 0;
  while (j + 2 < kk && m >= kn[j + 1]) ++j;
  const double h = kn[j + 1] - kn[j], xm = kn[j + 1] - m, xp = m - kn[j];
  const double am = xm / h, ap = xp / h;
  const double cm = (xm * xm * xm / h - h * xm) / 6.0, cp = (xp * xp * xp / h - h * xp) / 6.0;
  for (int i = 0; i < kk; ++i) row[i] = cm * F[j * KM + i] + cp * F[(j + 1) * KM + i];
  row[j] += am;
  row[j + 1] += ap;
}

__global__ __launch_bounds__(256) void k_od_valid(int64_t G, const double* __restrict__ m, const double* __restrict__ var, const int32_t* __restrict__ nobs,
                                                  int32_t min_cells, double* __restrict__ v, int32_t* __restrict__ valid) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  const double lv = log(var[g]);
  v[g] = lv;
  valid[g] = (isfinite(lv) && isfinite(m[g]) && nobs[g] >= min_cells) ? 1 : 0;
}

// the inclusive scan of one int per thread over the workgroup; s: 256 ints
__device__ inline int od_block_scan(int x, int* s) {
  const int t = threadIdx.x;
  __syncthreads();
  s[t] = x;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const int o = t >= d ? s[t - d] : 0;
    __syncthreads();
    s[t] += o;
    __syncthreads();
  }
  return s[t];
}

// One workgroup.  ux: the distinct m of the valid genes ascending; basis: n, u, kk, knots, F.
__global__ __launch_bounds__(256) void k_od_knots(int64_t G, const int32_t* __restrict__ count, const uint32_t* __restrict__ oval,
                                                  const double* __restrict__ m, int gam_k, double* __restrict__ ux, double* __restrict__ basis) {
#pragma clang fp contract(off)
  __shared__ int s_scan[256];
  const int t = threadIdx.x;
  int64_t n = count[0];
  if (n < 0) n = 0;
  if (n > G) n = G;
  int64_t u = 0;
  for (int64_t base = 0; base < n; base += 256) {
    const int64_t i = base + t;
    int flag = 0;
    double x = 0.0;
    if (i < n) {
      const uint32_t p = oval[i];
      x = p < (uint64_t)G ? m[p] : 0.0;
      flag = 1;
      if (i > 0) {
        const uint32_t pp = oval[i - 1];
        if (pp < (uint64_t)G && m[pp] == x) flag = 0;
      }
    }
    const int incl = od_block_scan(flag, s_scan);
    if (flag) ux[u + incl - 1] = x;
    u += s_scan[255];
  }
  __syncthreads();
  if (t != 0) return;
  int kk = gam_k;
  if ((double)n < 1.5 * (double)gam_k || gam_k < 2 || u < gam_k) kk = u >= 2 ? 2 : 1;
  double kn[KM], F[KM * KM];
  for (int j = 0; j < KM; ++j) kn[j] = 0.0;
  if (n >= 1) {
    if (kk == 1) kn[0] = ux[0];
    for (int j = 0; j < kk && kk >= 2; ++j) {
      const double tt = (double)j * (double)(u - 1) / (double)(kk - 1);
      int64_t lo = (int64_t)floor(tt), hi = (int64_t)ceil(tt);
      if (lo > u - 1) lo = u - 1;
      if (hi > u - 1) hi = u - 1;
      const double fr = tt - (double)lo;
      kn[j] = lo == hi ? ux[lo] : ux[lo] + fr * (ux[hi] - ux[lo]);
    }
    if (kk >= 2) { kn[0] = ux[0]; kn[kk - 1] = ux[u - 1]; }
  } else {
    kk = 0;
  }
  od_basis_F(kk, kn, F);
  basis[0] = (double)n;
  basis[1] = (double)u;
  basis[2] = (double)kk;
  for (int j = 0; j < KM; ++j) basis[3 + j] = kn[j];
  for (int j = 0; j < KM * KM; ++j) basis[3 + KM + j] = F[j];
}

// workgroup b of nb adds, in thread t, the genes b * 256 + t, + nb * 256, ... in turn; part[b]: the folded sum
__global__ __launch_bounds__(256) void k_od_sum_v(int64_t G, const double* __restrict__ v, const int32_t* __restrict__ valid, double* __restrict__ part) {
  __shared__ double s_fold[256];
  double a = 0.0;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < G; g += (int64_t)gridDim.x * 256)
    if (valid[g]) a += v[g];
  const double s = gficf_block_sum_f64(a, s_fold);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// One workgroup: out[s] = the folded sum over b < nb (<= 256) of part[b * ns + s]
__global__ __launch_bounds__(256) void k_od_fold(int nb, int ns, const double* __restrict__ part, double* __restrict__ out) {
  __shared__ double s_fold[256];
  for (int s = 0; s < ns; ++s) {
    const double a = (int)threadIdx.x < nb ? part[(int64_t)threadIdx.x * ns + s] : 0.0;
    const double r = gficf_block_sum_f64(a, s_fold);
    if (threadIdx.x == 0) out[s] = r;
  }
}

__global__ __launch_bounds__(256) void k_od_sums(int64_t G, const double* __restrict__ m, const double* __restrict__ v, const int32_t* __restrict__ valid,
                                                 const double* __restrict__ basis, const double* __restrict__ vsum, double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double s_fold[256];
  const int kk = (int)basis[2];
  const double vbar = vsum[0] / basis[0];
  double acc[OD_NS];
#pragma unroll
  for (int s = 0; s < OD_NS; ++s) acc[s] = 0.0;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < G; g += (int64_t)gridDim.x * 256) {
    if (!valid[g]) continue;
    double row[KM];
    od_row(kk, basis + 3, basis + 3 + KM, m[g], row);
    const double d = v[g] - vbar;
    acc[0] += d * d;
    int s = 1;
#pragma unroll
    for (int i = 0; i < KM; ++i)
#pragma unroll
      for (int j = i; j < KM; ++j) acc[s++] += row[i] * row[j];
#pragma unroll
    for (int i = 0; i < KM; ++i) acc[s++] += row[i] * d;
  }
#pragma unroll
  for (int s = 0; s < OD_NS; ++s) {
    const double r = gficf_block_sum_f64(acc[s], s_fold);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.x * OD_NS + s] = r;
  }
}

// coef: vbar, then beta (KM)
__global__ __launch_bounds__(256) void k_od_fit(int64_t G, const double* __restrict__ m, const double* __restrict__ v, const int32_t* __restrict__ valid,
                                                const double* __restrict__ basis, const double* __restrict__ coef, double* __restrict__ fit,
                                                double* __restrict__ res) {
#pragma clang fp contract(off)
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  if (!valid[g]) {
    fit[g] = __longlong_as_double(0x7ff8000000000000ll);
    res[g] = -__longlong_as_double(0x7ff0000000000000ll);
    return;
  }
  double row[KM];
  od_row((int)basis[2], basis + 3, basis + 3 + KM, m[g], row);
  double a = 0.0;
  for (int i = 0; i < KM; ++i) a += row[i] * coef[1 + i];
  const double f = coef[0] + a;
  fit[g] = f;
  res[g] = v[g] - f;
}

// ------------------------------------------------------- the two special functions
__device__ inline double od_softplus(double x) { return x > 0.0 ? x + log1p(exp(-x)) : log1p(exp(x)); }

// log I_z(a, a) at z = 1 / (1 + e^res): pf(exp(res), 2a, 2a, lower.tail = FALSE, log.p = TRUE)
__device__ inline double od_logpf(double res, double a, uint32_t* status) {
#pragma clang fp contract(off)
  const double nan = __longlong_as_double(0x7ff8000000000000ll), inf = __longlong_as_double(0x7ff0000000000000ll);
  if (!(a > 0.0) || !(res == res)) return nan;
  if (res == -inf) return 0.0;
  if (res == inf) return -inf;
  const double r = fabs(res);
  const double z = 1.0 / (1.0 + exp(r));
  // the continued fraction of the incomplete beta at (a, a, z), z <= 1/2, by the modified Lentz method
  const double tiny = 1e-300, qab = a + a, qap = a + 1.0, qam = a - 1.0;
  double c = 1.0, d = 1.0 - qab * z / qap;
  if (fabs(d) < tiny) d = tiny;
  d = 1.0 / d;
  double h = d;
  int it = 1;
  for (; it <= OD_CF_CAP; ++it) {
    const double mm = (double)it, m2 = mm + mm;
    double aa = mm * (a - mm) * z / ((qam + m2) * (a + m2));
    d = 1.0 + aa * d;
    if (fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    h = h * (d * c);
    aa = -(a + mm) * (qab + mm) * z / ((a + m2) * (qap + m2));
    d = 1.0 + aa * d;
    if (fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    h = h * del;
    if (fabs(del - 1.0) < 2e-15) break;
  }
  if (it > OD_CF_CAP) atomicOr(status, OD_ST_ITER);
  const double lz = -od_softplus(r), l1z = -od_softplus(-r);
  const double lp = a * (lz + l1z) - log(a) - (2.0 * lgamma(a) - lgamma(a + a)) + log(h);
  if (res >= 0.0) return lp;
  return log1p(-exp(lp));
}

// log P(a, y) and log Q(a, y), the regularised incomplete gammas: the series of P below a + 1, the Legendre continued fraction of Q
// above; the other one from its complement
__device__ inline void od_logPQ(double a, double y, double* lP, double* lQ, uint32_t* status) {
#pragma clang fp contract(off)
  const double ln2 = 0.6931471805599453;
  const double front = a * log(y) - y;
  if (y < a + 1.0) {
    double ap = a, del = 1.0, sum = 1.0;
    int it = 1;
    for (; it <= OD_CF_CAP; ++it) {
      ap = ap + 1.0;
      del = del * (y / ap);
      sum = sum + del;
      if (del < sum * 1e-16) break;
    }
    if (it > OD_CF_CAP) atomicOr(status, OD_ST_ITER);
    const double p = front - lgamma(a + 1.0) + log(sum);
    *lP = p;
    *lQ = p < -ln2 ? log1p(-exp(p)) : log(-expm1(p));
    return;
  }
  const double tiny = 1e-300;
  double b = y + 1.0 - a, c = 1.0 / tiny, d = 1.0 / b, h = d;
  int it = 1;
  for (; it <= OD_CF_CAP; ++it) {
    const double an = -(double)it * ((double)it - a);
    b = b + 2.0;
    d = an * d + b;
    if (fabs(d) < tiny) d = tiny;
    c = b + an / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    h = h * del;
    if (fabs(del - 1.0) < 2e-15) break;
  }
  if (it > OD_CF_CAP) atomicOr(status, OD_ST_ITER);
  const double q = front - lgamma(a) + log(h);
  *lQ = q;
  *lP = q < -ln2 ? log1p(-exp(q)) : log(-expm1(q));
}

// the x with log Q(df / 2, x / 2) = lp: qchisq(lp, df, lower.tail = FALSE, log.p = TRUE).  Newton on the smaller tail, bracketed:
// in y on log Q where the upper tail is the smaller one, in log y on log P (nearly a straight line there) where the lower one is
__device__ inline double od_logqchisq(double lp, double df, uint32_t* status) {
#pragma clang fp contract(off)
  const double nan = __longlong_as_double(0x7ff8000000000000ll), inf = __longlong_as_double(0x7ff0000000000000ll);
  if (!(df > 0.0) || !(lp == lp) || lp > 0.0) return nan;
  if (lp == 0.0) return 0.0;
  if (lp == -inf) return inf;
  const double a = 0.5 * df, lga = lgamma(a);
  // the start: Wilson-Hilferty from a rational normal quantile (Abramowitz & Stegun 26.2.23), or the first term of P's series
  const double lq = lp < -0.6931471805599453 ? log1p(-exp(lp)) : log(-expm1(lp));     // log P
  const bool upper = lp <= lq;                                                        // the upper tail is the smaller one
  const double t0 = sqrt(-2.0 * (upper ? lp : lq));
  double zq = t0 - (2.515517 + t0 * (0.802853 + t0 * 0.010328)) / (1.0 + t0 * (1.432788 + t0 * (0.189269 + t0 * 0.001308)));
  if (!upper) zq = -zq;
  const double cc = 2.0 / (9.0 * df), w = 1.0 - cc + zq * sqrt(cc);
  double y = 0.5 * df * w * w * w;
  const double ys = exp((lq + lgamma(a + 1.0)) / a);
  if (!(w > 0.0) || !(y > 0.0) || ys < 0.05 * (a + 1.0)) y = ys;
  if (!(y > 0.0) || !isfinite(y)) y = a;
  double prev = inf;
  int it = 0;
  if (upper) {
    double lo = 0.0, hi = inf;
    for (; it < OD_NEWTON_CAP; ++it) {
      double lP, lQ;
      od_logPQ(a, y, &lP, &lQ, status);
      const double f = lQ - lp;
      if (f == 0.0) break;
      if (f > 0.0) lo = y; else hi = y;
      const double hz = exp((a - 1.0) * log(y) - y - lga - lQ);                        // -d log Q / dy
      double yn = y + f / hz;
      if (yn > 0.0 && fabs(yn - y) <= 1e-13 * y) { y = yn; break; }                    // converged
      if (!(yn > lo) || !(yn < hi) || !isfinite(yn)) yn = hi == inf ? 2.0 * y : (lo > 0.0 ? sqrt(lo) * sqrt(hi) : 0.5 * hi);
      const double dy = fabs(yn - y);
      y = yn;
      if (dy >= prev && prev <= 1e-9 * y) break;                                       // down to the rounding of log Q
      prev = dy;
    }
  } else {
    double t = log(y), lo = -inf, hi = inf;
    for (; it < OD_NEWTON_CAP; ++it) {
      double lP, lQ;
      y = exp(t);
      od_logPQ(a, y, &lP, &lQ, status);
      const double g = lP - lq;
      if (g == 0.0) break;
      if (g < 0.0) lo = t; else hi = t;
      const double sl = exp(a * t - y - lga - lP);                                     // d log P / d log y
      double tn = t - g / sl;
      if (fabs(tn - t) <= 1e-13) { t = tn; break; }                                    // converged
      if (!(tn > lo) || !(tn < hi) || !isfinite(tn)) tn = lo == -inf ? t - 1.0 : (hi == inf ? t + 1.0 : 0.5 * (lo + hi));
      const double dt = fabs(tn - t);
      t = tn;
      if (dt >= prev && prev <= 1e-9) break;
      prev = dt;
    }
    y = exp(t);
  }
  if (it >= OD_NEWTON_CAP) atomicOr(status, OD_ST_ITER);
  return 2.0 * y;
}

__global__ __launch_bounds__(256) void k_od_logpf(int64_t n, const double* __restrict__ res, const double* __restrict__ a, double* __restrict__ lp,
                                                  uint32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) lp[i] = od_logpf(res[i], a[i], status);
}

__global__ __launch_bounds__(256) void k_od_logqchisq(int64_t n, const double* __restrict__ lp, double df, double* __restrict__ x,
                                                      uint32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] = od_logqchisq(lp[i], df, status);
}

__global__ __launch_bounds__(256) void k_od_scores(int64_t G, const double* __restrict__ res, const int32_t* __restrict__ nobs, const double* __restrict__ v,
                                                   double N, double min_av, double max_av, double* __restrict__ lp, double* __restrict__ qv,
                                                   double* __restrict__ gsf, uint32_t* __restrict__ status) {
#pragma clang fp contract(off)
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  const double l = od_logpf(res[g], 0.5 * (double)nobs[g], status);
  const double q = od_logqchisq(l, N - 1.0, status) / N;
  lp[g] = l;
  qv[g] = q;
  double c = q;                                            // pmax(min, pmin(max, qv)): a NaN stays
  if (c > max_av) c = max_av;
  if (c < min_av) c = min_av;
  double s = sqrt(c / exp(v[g]));
  if (!isfinite(s)) s = 0.0;
  gsf[g] = s;
}

__global__ __launch_bounds__(256) void k_od_notnan(int64_t n, const double* __restrict__ lp, int32_t* __restrict__ mask) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) mask[i] = lp[i] == lp[i] ? 1 : 0;
}

// One workgroup.  oval: the order of lp (the NaN last); n: how many are not NaN; lg[i] = log(n / (i + 1)).
// q_i = lp_(i) + lg[i]; the running minimum from the end, by chunks of 256 from the last; scattered back.
__global__ __launch_bounds__(256) void k_od_bh(int64_t G, int64_t n, const uint32_t* __restrict__ oval, const double* __restrict__ lp,
                                               const double* __restrict__ lg, double* __restrict__ lpa) {
#pragma clang fp contract(off)
  __shared__ double s_q[256];
  const int t = threadIdx.x;
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  for (int64_t i = n + t; i < G; i += 256) {
    const uint32_t p = oval[i];
    if (p < (uint64_t)G) lpa[p] = lp[p];                   // a NaN stays
  }
  double carry = inf;
  const int64_t chunks = gficf_ceil_div(n, 256);
  for (int64_t c = chunks - 1; c >= 0; --c) {
    const int64_t i = c * 256 + t;
    uint32_t p = 0;
    double q = inf;
    if (i < n) {
      p = oval[i];
      if (p < (uint64_t)G) q = lp[p] + lg[i];
    }
    __syncthreads();
    s_q[t] = q;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {                    // the suffix minimum within the chunk
      const double o = t + d < 256 ? s_q[t + d] : inf;
      __syncthreads();
      s_q[t] = fmin(s_q[t], o);
      __syncthreads();
    }
    const double r = fmin(s_q[t], carry);
    if (i < n && p < (uint64_t)G) lpa[p] = r;
    carry = fmin(carry, s_q[0]);
  }
}

// ------------------------------------------------------- rows selected and scaled
// One workgroup: newid[g] = the selected rows before g (its new number where mask[g] != 0); nsel[0] = how many are selected
__global__ __launch_bounds__(256) void k_od_newid(int64_t G, const int32_t* __restrict__ mask, int32_t* __restrict__ newid, int32_t* __restrict__ nsel) {
  __shared__ int s_scan[256];
  const int t = threadIdx.x;
  int64_t carry = 0;
  for (int64_t base = 0; base < G; base += 256) {
    const int64_t g = base + t;
    const int f = (g < G && mask[g] != 0) ? 1 : 0;
    const int incl = od_block_scan(f, s_scan);
    if (g < G) newid[g] = (int32_t)(carry + incl - f);
    carry += s_scan[255];
  }
  if (t == 0) nsel[0] = (int32_t)carry;
}

__device__ inline bool od_col_range(const int64_t* colptr, int64_t c, int64_t nnz, int64_t* beg, int64_t* end, uint32_t* status) {
  int64_t b = colptr[c], e = colptr[c + 1];
  bool ok = true;
  if (b < 0 || e > nnz || e < b) {
    ok = false;
    atomicOr(status, OD_ST_CSC);
    if (b < 0) b = 0;
    if (e > nnz) e = nnz;
    if (e < b) e = b;
  }
  *beg = b;
  *end = e;
  return ok;
}

// One wave per column: cnt[c] = its entries in selected rows
__global__ __launch_bounds__(256) void k_od_count(int64_t G, int64_t N, int64_t nnz, const int64_t* __restrict__ colptr, const int32_t* __restrict__ rowidx,
                                                  const int32_t* __restrict__ mask, int64_t* __restrict__ cnt, uint32_t* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (c >= N) return;                                      // the whole wave
  int64_t beg, end;
  od_col_range(colptr, c, nnz, &beg, &end, status);
  int k = 0;
  for (int64_t p = beg + lane; p < end; p += 64) {
    const int32_t r = rowidx[p];
    if (r < 0 || r >= G) atomicOr(status, OD_ST_CSC);
    else if (mask[r] != 0) ++k;
  }
  k = gficf_wave_sum(k);
  if (lane == 0) cnt[c] = k;
}

// One workgroup: out[c] = cnt[0] + ... + cnt[c - 1], c = 0 .. N
__global__ __launch_bounds__(256) void k_od_colscan(int64_t N, const int64_t* __restrict__ cnt, int64_t* __restrict__ out) {
  __shared__ int s_scan[256];
  const int t = threadIdx.x;
  int64_t carry = 0;
  if (t == 0) out[0] = 0;
  for (int64_t base = 0; base < N; base += 256) {
    const int64_t c = base + t;
    const int k = c < N ? (int)cnt[c] : 0;                 // a column holds at most G < 2^31 / 64 selected rows
    const int incl = od_block_scan(k, s_scan);
    if (c < N) out[c + 1] = carry + incl;
    carry += s_scan[255];
  }
}

// One wave per column: its entries in selected rows, in order, renumbered and scaled, from out_colptr[c] on (never beyond cap)
__global__ __launch_bounds__(256) void k_od_write(int64_t G, int64_t N, int64_t nnz, const int64_t* __restrict__ colptr, const int32_t* __restrict__ rowidx,
                                                  const double* __restrict__ x, const int32_t* __restrict__ mask, const int32_t* __restrict__ newid,
                                                  const double* __restrict__ scale, const int64_t* __restrict__ out_colptr, int64_t cap,
                                                  int32_t* __restrict__ out_rowidx, double* __restrict__ out_x, uint32_t* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (c >= N) return;                                      // the whole wave
  int64_t beg, end;
  od_col_range(colptr, c, nnz, &beg, &end, status);
  int64_t at = out_colptr[c];
  for (int64_t base = beg; base < end; base += 64) {
    const int64_t p = base + lane;
    int32_t r = -1;
    if (p < end) r = rowidx[p];
    const bool keep = r >= 0 && r < G && mask[r] != 0;
    const unsigned long long bal = __ballot(keep);
    if (keep) {
      const int64_t o = at + __popcll(bal & ((1ull << lane) - 1ull));
      if (o >= 0 && o < cap) {
        out_rowidx[o] = newid[r];
        out_x[o] = scale ? x[p] * scale[r] : x[p];
      } else {
        atomicOr(status, OD_ST_CSC);
      }
    }
    at += __popcll(bal);
  }
}

__global__ __launch_bounds__(256) void k_od_scale(int64_t G, int64_t nnz, const int32_t* __restrict__ rowidx, const double* __restrict__ x,
                                                  const double* __restrict__ scale, double* __restrict__ out_x, uint32_t* __restrict__ status) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * 256) {
    const int32_t r = rowidx[p];
    if (r < 0 || r >= G) { atomicOr(status, OD_ST_CSC); out_x[p] = x[p]; continue; }
    out_x[p] = scale ? x[p] * scale[r] : x[p];
  }
}

// ------------------------------------------------------- workspace
struct OdWs {
  uint32_t* status;
  int32_t* count;
  gficf_sort_bufs sort;
  int32_t *mask, *newid;
  double *ux, *lg, *basis, *part, *sums, *coef;
  int64_t* cnt;
};

static size_t od_carve(char* base, int64_t G, int64_t N, OdWs& w) {
  gficf_carver cv;
  cv.base = base;
  const size_t g1 = (size_t)(G > 0 ? G : 1);
  w.status = cv.take<uint32_t>(1);
  w.count = cv.take<int32_t>(1);
  w.sort.take(cv, g1, g1, {});
  w.mask = cv.take<int32_t>(g1);
  w.newid = cv.take<int32_t>(g1);
  w.ux = cv.take<double>(g1);
  w.lg = cv.take<double>(g1);
  w.basis = cv.take<double>(OD_BASIS);
  w.part = cv.take<double>((size_t)256 * OD_NS);
  w.sums = cv.take<double>(1 + OD_NS);
  w.coef = cv.take<double>(1 + KM);
  w.cnt = cv.take<int64_t>((size_t)(N > 0 ? N : 0) + 1);
  return cv.total();
}

static bool od_sizes_ok(int64_t G, int64_t N) { return G >= 1 && G <= (int64_t)INT32_MAX / 64 && N >= 0 && N <= INT32_MAX; }

static int od_workspace(void* ws, size_t ws_bytes, int64_t G, int64_t N, OdWs& w) {
  if (!ws) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL workspace");
  if (!od_sizes_ok(G, N)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "G = %lld, N = %lld: a size is out of range", (long long)G, (long long)N);
  return gficf_addon_carve(ws, ws_bytes, [&](char* base) { return od_carve(base, G, N, w); });
}

static unsigned od_grid(int64_t n) { return (unsigned)gficf_ceil_div(n > 0 ? n : 1, 256); }
static unsigned od_waves(int64_t n) { return (unsigned)gficf_ceil_div(n > 0 ? n : 1, 4); }
static unsigned od_parts(int64_t n) { return gficf_grid_capped(n, 256, 256); }

// ------------------------------------------------------- the k x k stage (host, plain f64)
struct OdModel {
  int kk;
  double n, u, vbar, lambda, gcv, edf, rss;
  double kn[KM], beta[KM];
};

struct OdSpec {                                            // the spectrum the GCV score is a function of
  int kk;
  double n, syy, s[KM], z[KM];
};

static void od_gcv_at(const OdSpec& sp, double lambda, double* gcv, double* edf, double* rss) {
#pragma clang fp contract(off)
  double tr = 0.0, fitted = 0.0;
  for (int i = 0; i < sp.kk; ++i) {
    const double g = sp.s[i] == 0.0 ? 1.0 : 1.0 / (1.0 + lambda * sp.s[i]);
    tr += g;
    fitted += sp.z[i] * sp.z[i] * (2.0 * g - g * g);
  }
  const double r = sp.syy - fitted, den = sp.n - tr;
  *edf = tr;
  *rss = r;
  *gcv = den > 0.0 ? sp.n * r / (den * den) : std::numeric_limits<double>::infinity();
}

static double od_gcv_rho(const OdSpec& sp, double rho) {
  double g, e, r;
  od_gcv_at(sp, std::exp(rho), &g, &e, &r);
  return g;
}

// sums: sum (v - vbar)^2, X^T X (upper triangle by rows, stride KM), X^T (v - vbar); sp_fixed < 0 (or NaN): the GCV search
static int od_solve(const double* sums, double sp_fixed, OdModel& md) {
#pragma clang fp contract(off)
  const int kk = md.kk;
  double A[KM][KM], b[KM], S[KM][KM], F[KM * KM];
  {
    int s = 1;
    for (int i = 0; i < KM; ++i)
      for (int j = i; j < KM; ++j) { A[i][j] = sums[s]; A[j][i] = sums[s]; ++s; }
    for (int i = 0; i < KM; ++i) b[i] = sums[s++];
  }
  // the penalty S = D^T B^-1 D = D^T (rows 1 .. kk - 2 of F)
  od_basis_F(kk, md.kn, F);
  for (int i = 0; i < KM; ++i)
    for (int j = 0; j < KM; ++j) S[i][j] = 0.0;
  for (int i = 0; i + 2 < kk; ++i) {
    const double h0 = md.kn[i + 1] - md.kn[i], h1 = md.kn[i + 2] - md.kn[i + 1];
    const double dv[3] = {1.0 / h0, -1.0 / h0 - 1.0 / h1, 1.0 / h1};
    for (int a = 0; a < 3; ++a)
      for (int c = 0; c < kk; ++c) S[i + a][c] += dv[a] * F[(i + 1) * KM + c];
  }
  for (int i = 0; i < kk; ++i)
    for (int j = i + 1; j < kk; ++j) { const double t = 0.5 * (S[i][j] + S[j][i]); S[i][j] = t; S[j][i] = t; }
  // X^T X = L L^T
  double L[KM][KM] = {};
  for (int j = 0; j < kk; ++j) {
    double d = A[j][j];
    for (int p = 0; p < j; ++p) d -= L[j][p] * L[j][p];
    if (!(d > 0.0) || !std::isfinite(d)) GFICF_FAIL(GFICF_ERR_BAD_VALUE, "the variance fit is singular: X^T X is not positive definite at column %d of %d", j, kk);
    L[j][j] = std::sqrt(d);
    for (int i = j + 1; i < kk; ++i) {
      double t = A[i][j];
      for (int p = 0; p < j; ++p) t -= L[i][p] * L[j][p];
      L[i][j] = t / L[j][j];
    }
  }
  // M = L^-1 S L^-T
  double T[KM][KM] = {}, M[KM][KM] = {}, U[KM][KM] = {};
  for (int c = 0; c < kk; ++c)
    for (int i = 0; i < kk; ++i) {
      double t = S[i][c];
      for (int p = 0; p < i; ++p) t -= L[i][p] * T[p][c];
      T[i][c] = t / L[i][i];
    }
  for (int r = 0; r < kk; ++r)                              // row r of M solves L M[r]^T = T[r]^T
    for (int i = 0; i < kk; ++i) {
      double t = T[r][i];
      for (int p = 0; p < i; ++p) t -= L[i][p] * M[r][p];
      M[r][i] = t / L[i][i];
    }
  for (int i = 0; i < kk; ++i)
    for (int j = i + 1; j < kk; ++j) { const double t = 0.5 * (M[i][j] + M[j][i]); M[i][j] = t; M[j][i] = t; }
  // cyclic Jacobi: M = U diag(s) U^T
  for (int i = 0; i < kk; ++i) U[i][i] = 1.0;
  for (int sweep = 0; sweep < 100; ++sweep) {
    double off = 0.0, dg = 0.0;
    for (int i = 0; i < kk; ++i) {
      dg += M[i][i] * M[i][i];
      for (int j = i + 1; j < kk; ++j) off += M[i][j] * M[i][j];
    }
    if (off <= 1e-60 * dg || off == 0.0) break;
    for (int p = 0; p < kk; ++p)
      for (int q = p + 1; q < kk; ++q) {
        if (M[p][q] == 0.0) continue;
        const double th = (M[q][q] - M[p][p]) / (2.0 * M[p][q]);
        const double t = (th >= 0.0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int i = 0; i < kk; ++i) {
          const double a = M[i][p], bq = M[i][q];
          M[i][p] = c * a - s * bq;
          M[i][q] = s * a + c * bq;
        }
        for (int i = 0; i < kk; ++i) {
          const double a = M[p][i], bq = M[q][i];
          M[p][i] = c * a - s * bq;
          M[q][i] = s * a + c * bq;
        }
        for (int i = 0; i < kk; ++i) {
          const double a = U[i][p], bq = U[i][q];
          U[i][p] = c * a - s * bq;
          U[i][q] = s * a + c * bq;
        }
      }
  }
  int ord[KM];
  for (int i = 0; i < kk; ++i) ord[i] = i;
  std::stable_sort(ord, ord + kk, [&](int a, int c) { return M[a][a] < M[c][c]; });
  OdSpec spx;
  spx.kk = kk;
  spx.n = md.n;
  spx.syy = sums[0];
  double r[KM];
  for (int i = 0; i < kk; ++i) {
    double t = b[i];
    for (int p = 0; p < i; ++p) t -= L[i][p] * r[p];
    r[i] = t / L[i][i];
  }
  for (int e = 0; e < kk; ++e) {
    const int col = ord[e];
    double sv = M[col][col];
    if (e < 2 || !(sv > 0.0)) sv = 0.0;                    // the penalty's null space: constants and straight lines
    spx.s[e] = sv;
    double z = 0.0;
    for (int i = 0; i < kk; ++i) z += U[i][col] * r[i];
    spx.z[e] = z;
  }
  double lambda;
  if (sp_fixed >= 0.0) {
    lambda = sp_fixed;
  } else {
    const double ln10 = std::log(10.0);
    int best = 0;
    double gbest = std::numeric_limits<double>::infinity();
    for (int j = 0; j < 97; ++j) {
      const double g = od_gcv_rho(spx, ln10 * (-12.0 + (double)j / 4.0));
      if (g < gbest) { gbest = g; best = j; }
    }
    double rho = ln10 * (-12.0 + (double)best / 4.0);
    if (best > 0 && best < 96) {
      const double phi = (std::sqrt(5.0) - 1.0) / 2.0;
      double lo = ln10 * (-12.0 + (double)(best - 1) / 4.0), hi = ln10 * (-12.0 + (double)(best + 1) / 4.0);
      double c = hi - phi * (hi - lo), d = lo + phi * (hi - lo);
      double fc = od_gcv_rho(spx, c), fd = od_gcv_rho(spx, d);
      for (int it = 0; it < 60; ++it) {
        if (fc < fd) {
          hi = d; d = c; fd = fc;
          c = hi - phi * (hi - lo);
          fc = od_gcv_rho(spx, c);
        } else {
          lo = c; c = d; fc = fd;
          d = lo + phi * (hi - lo);
          fd = od_gcv_rho(spx, d);
        }
      }
      rho = 0.5 * (lo + hi);
    }
    lambda = std::exp(rho);
  }
  md.lambda = lambda;
  od_gcv_at(spx, lambda, &md.gcv, &md.edf, &md.rss);
  // beta = L^-T U (gamma z)
  double y[KM] = {};
  for (int e = 0; e < kk; ++e) {
    const double g = spx.s[e] == 0.0 ? 1.0 : 1.0 / (1.0 + lambda * spx.s[e]);
    const double gz = g * spx.z[e];
    for (int i = 0; i < kk; ++i) y[i] += U[i][ord[e]] * gz;
  }
  for (int i = 0; i < KM; ++i) md.beta[i] = 0.0;
  for (int i = kk - 1; i >= 0; --i) {
    double t = y[i];
    for (int p = i + 1; p < kk; ++p) t -= L[p][i] * md.beta[p];
    md.beta[i] = t / L[i][i];
  }
  return GFICF_OK;
}

static void od_info(const OdModel& md, double* info) {
  info[0] = md.n; info[1] = md.u; info[2] = (double)md.kk; info[3] = md.lambda; info[4] = md.gcv; info[5] = md.edf; info[6] = md.vbar; info[7] = md.rss;
  for (int j = 0; j < KM; ++j) info[8 + j] = j < md.kk ? md.kn[j] : std::numeric_limits<double>::quiet_NaN();
}

static int od_fit(gficf_ctx* ctx, const OdWs& w, int64_t G, const double* d_m, const double* d_var, const int32_t* d_nobs, int32_t gam_k,
                  int32_t min_cells, double sp, double* d_v, int32_t* d_valid, double* d_fit, double* d_res, double* info) {
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(k_od_valid, dim3(od_grid(G)), dim3(256), 0, st, G, d_m, d_var, d_nobs, min_cells, d_v, d_valid);
  GFICF_HIP_CHECK(hipMemsetAsync(w.count, 0, sizeof(int32_t), st));
  int rc = gficf_sort_f64(ctx, w.sort, G, {d_m, 0, d_valid, nullptr, 0u, w.count, nullptr, 0u, 0});
  if (rc) return rc;
  hipLaunchKernelGGL(k_od_knots, dim3(1), dim3(256), 0, st, G, (const int32_t*)w.count, (const uint32_t*)w.sort.oval, d_m, (int)gam_k, w.ux, w.basis);
  const unsigned nb = od_parts(G);
  hipLaunchKernelGGL(k_od_sum_v, dim3(nb), dim3(256), 0, st, G, (const double*)d_v, (const int32_t*)d_valid, w.part);
  hipLaunchKernelGGL(k_od_fold, dim3(1), dim3(256), 0, st, (int)nb, 1, (const double*)w.part, w.sums);
  hipLaunchKernelGGL(k_od_sums, dim3(nb), dim3(256), 0, st, G, d_m, (const double*)d_v, (const int32_t*)d_valid, (const double*)w.basis,
                     (const double*)w.sums, w.part);
  hipLaunchKernelGGL(k_od_fold, dim3(1), dim3(256), 0, st, (int)nb, OD_NS, (const double*)w.part, w.sums + 1);
  GFICF_HIP_CHECK(hipGetLastError());
  double basis[3 + KM], sums[1 + OD_NS];
  GFICF_HIP_CHECK(hipMemcpyAsync(basis, w.basis, sizeof(basis), hipMemcpyDeviceToHost, st));
  GFICF_HIP_CHECK(hipMemcpyAsync(sums, w.sums, sizeof(sums), hipMemcpyDeviceToHost, st));
  GFICF_RC(gficf_ctx_sync(ctx));
  OdModel md = {};
  md.n = basis[0];
  md.u = basis[1];
  md.kk = (int)basis[2];
  for (int j = 0; j < KM; ++j) md.kn[j] = basis[3 + j];
  const double nan = std::numeric_limits<double>::quiet_NaN();
  md.lambda = md.gcv = md.edf = md.rss = md.vbar = nan;
  double coef[1 + KM] = {};
  if (md.kk >= 1) {
    md.vbar = sums[0] / md.n;
    rc = od_solve(sums + 1, sp, md);
    if (rc) return rc;
    coef[0] = md.vbar;
    for (int j = 0; j < KM; ++j) coef[1 + j] = md.beta[j];
  }
  if (info) od_info(md, info);
  GFICF_HIP_CHECK(hipMemcpyAsync(w.coef, coef, sizeof(coef), hipMemcpyHostToDevice, st));
  GFICF_HIP_CHECK(hipStreamSynchronize(st));               // coef lives on this frame
  hipLaunchKernelGGL(k_od_fit, dim3(od_grid(G)), dim3(256), 0, st, G, d_m, (const double*)d_v, (const int32_t*)d_valid, (const double*)w.basis,
                     (const double*)w.coef, d_fit, d_res);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

static int od_bh(gficf_ctx* ctx, const OdWs& w, int64_t G, const double* d_lp, double* d_lpa) {
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(k_od_notnan, dim3(od_grid(G)), dim3(256), 0, st, G, d_lp, w.mask);
  GFICF_HIP_CHECK(hipMemsetAsync(w.count, 0, sizeof(int32_t), st));
  int rc = gficf_sort_f64(ctx, w.sort, G, {d_lp, 0, w.mask, nullptr, 0u, w.count, nullptr, 0u, 0});
  if (rc) return rc;
  int32_t n32 = 0;
  GFICF_HIP_CHECK(hipMemcpyAsync(&n32, w.count, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  GFICF_RC(gficf_ctx_sync(ctx));
  const int64_t n = n32 < 0 ? 0 : (n32 > G ? G : n32);
  // log(n / i) on the host: the operands of the adds are the C library's, whatever the device's log rounds to
  std::vector<double> lg((size_t)(n > 0 ? n : 1));
  for (int64_t i = 0; i < n; ++i) lg[(size_t)i] = std::log((double)n / (double)(i + 1));
  if (n > 0) GFICF_HIP_CHECK(hipMemcpyAsync(w.lg, lg.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
  GFICF_HIP_CHECK(hipStreamSynchronize(st));               // lg lives on this frame
  hipLaunchKernelGGL(k_od_bh, dim3(1), dim3(256), 0, st, G, n, (const uint32_t*)w.sort.oval, d_lp, (const double*)w.lg, d_lpa);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

static int od_scores(gficf_ctx* ctx, const OdWs& w, int64_t G, const double* d_res, const int32_t* d_nobs, const double* d_v, int64_t N, double min_av,
                     double max_av, double* d_lp, double* d_qv, double* d_gsf) {
  hipLaunchKernelGGL(k_od_scores, dim3(od_grid(G)), dim3(256), 0, ctx->stream, G, d_res, d_nobs, d_v, (double)N, min_av, max_av, d_lp, d_qv, d_gsf, w.status);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

static int od_check_k(int32_t gam_k) {
  if (gam_k == 2 || gam_k > KM) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "gam_k = %d: the cubic regression spline takes 3 to %d knots (below 2: the straight line)", gam_k, KM);
  return GFICF_OK;
}

struct OdOut {
  double *v, *fit, *res, *lp, *lpa, *qv, *gsf, *info;
  int32_t* valid;
};

// everything after the moments, from device lists; the stream is idle at the return
static int od_run(gficf_ctx* ctx, gficf_host_io& io, char* d_ws, size_t wsb, int64_t G, int64_t N, const double* d_m, const double* d_var,
                  const int32_t* d_nobs, int32_t gam_k, int32_t min_cells, double min_av, double max_av, double sp, double* d_out, const OdOut& o) {
  OdWs w;
  int rc = od_workspace(d_ws, wsb, G, 0, w);
  if (rc) return io.drain(rc);
  if (io.ok()) io.e = hipMemsetAsync(w.status, 0, sizeof(uint32_t), ctx->stream);
  if (!io.ok()) return io.drain(GFICF_OK);
  const size_t g = (size_t)G;
  double *d_v = d_out, *d_fit = d_out + g, *d_res = d_out + 2 * g, *d_lp = d_out + 3 * g, *d_lpa = d_out + 4 * g, *d_qv = d_out + 5 * g, *d_gsf = d_out + 6 * g;
  int32_t* d_valid = (int32_t*)(d_out + 7 * g);
  rc = od_fit(ctx, w, G, d_m, d_var, d_nobs, gam_k, min_cells, sp, d_v, d_valid, d_fit, d_res, o.info);
  if (!rc) rc = od_scores(ctx, w, G, d_res, d_nobs, d_v, N, min_av, max_av, d_lp, d_qv, d_gsf);
  if (!rc) rc = od_bh(ctx, w, G, d_lp, d_lpa);
  if (rc) return io.drain(rc);
  if (o.v) io.down(o.v, d_v, sizeof(double) * g);
  if (o.fit) io.down(o.fit, d_fit, sizeof(double) * g);
  if (o.res) io.down(o.res, d_res, sizeof(double) * g);
  if (o.lp) io.down(o.lp, d_lp, sizeof(double) * g);
  if (o.lpa) io.down(o.lpa, d_lpa, sizeof(double) * g);
  if (o.qv) io.down(o.qv, d_qv, sizeof(double) * g);
  if (o.gsf) io.down(o.gsf, d_gsf, sizeof(double) * g);
  if (o.valid) io.down(o.valid, d_valid, sizeof(int32_t) * g);
  if (!io.ok()) return io.drain(GFICF_OK);
  return gficf_od_sync(ctx, d_ws);
}

}  // namespace

extern "C" {

int gficf_od_abi_version(void) { return GFICF_OD_ABI_VERSION; }

size_t gficf_od_workspace_bytes(int64_t G, int64_t N) {
  if (!od_sizes_ok(G, N)) return 0;
  OdWs w;
  return od_carve(nullptr, G, N, w);
}

int gficf_od_fit_device(gficf_ctx* ctx, int64_t G, const double* d_m, const double* d_var, const int32_t* d_nobs, int32_t gam_k, int32_t min_gene_cells,
                        double sp, void* ws, size_t ws_bytes, double* d_v, int32_t* d_valid, double* d_fit, double* d_res, double* info) {
  GFICF_CTX_ENTER(ctx);
  if (!d_m || !d_var || !d_nobs || !d_v || !d_valid || !d_fit || !d_res) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  GFICF_RC(od_check_k(gam_k));
  OdWs w;
  GFICF_RC(od_workspace(ws, ws_bytes, G, 0, w));
  return od_fit(ctx, w, G, d_m, d_var, d_nobs, gam_k, min_gene_cells, sp, d_v, d_valid, d_fit, d_res, info);
}

int gficf_od_logpf_device(gficf_ctx* ctx, int64_t n, const double* d_res, const double* d_a, void* ws, size_t ws_bytes, double* d_lp) {
  GFICF_CTX_ENTER(ctx);
  if (!d_res || !d_a || !d_lp) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  OdWs w;
  GFICF_RC(od_workspace(ws, ws_bytes, n, 0, w));
  hipLaunchKernelGGL(k_od_logpf, dim3(od_grid(n)), dim3(256), 0, ctx->stream, n, d_res, d_a, d_lp, w.status);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int gficf_od_logqchisq_device(gficf_ctx* ctx, int64_t n, const double* d_lp, double df, void* ws, size_t ws_bytes, double* d_x) {
  GFICF_CTX_ENTER(ctx);
  if (!d_lp || !d_x) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  OdWs w;
  GFICF_RC(od_workspace(ws, ws_bytes, n, 0, w));
  hipLaunchKernelGGL(k_od_logqchisq, dim3(od_grid(n)), dim3(256), 0, ctx->stream, n, d_lp, df, d_x, w.status);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int gficf_od_scores_device(gficf_ctx* ctx, int64_t G, const double* d_res, const int32_t* d_nobs, const double* d_v, int64_t N, double min_adjusted_variance,
                           double max_adjusted_variance, void* ws, size_t ws_bytes, double* d_lp, double* d_qv, double* d_gsf) {
  GFICF_CTX_ENTER(ctx);
  if (!d_res || !d_nobs || !d_v || !d_lp || !d_qv || !d_gsf) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  if (N < 2) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "N = %lld: the adjusted variance needs at least 2 cells", (long long)N);
  OdWs w;
  GFICF_RC(od_workspace(ws, ws_bytes, G, 0, w));
  return od_scores(ctx, w, G, d_res, d_nobs, d_v, N, min_adjusted_variance, max_adjusted_variance, d_lp, d_qv, d_gsf);
}

int gficf_od_bh_log_device(gficf_ctx* ctx, int64_t G, const double* d_lp, void* ws, size_t ws_bytes, double* d_lpa) {
  GFICF_CTX_ENTER(ctx);
  if (!d_lp || !d_lpa) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  OdWs w;
  GFICF_RC(od_workspace(ws, ws_bytes, G, 0, w));
  return od_bh(ctx, w, G, d_lp, d_lpa);
}

int gficf_od_select_scale_device(gficf_ctx* ctx, int64_t G, int64_t N, const int64_t* d_colptr, const int32_t* d_rowidx, const double* d_x, int64_t nnz,
                                 const int32_t* d_mask, const double* d_scale, void* ws, size_t ws_bytes, int64_t* d_out_colptr, int32_t* d_out_rowidx,
                                 double* d_out_x, int32_t* d_nsel) {
  GFICF_CTX_ENTER(ctx);
  if (nnz < 0 || !d_colptr || (nnz > 0 && (!d_rowidx || !d_x || !d_out_x))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  OdWs w;
  GFICF_RC(od_workspace(ws, ws_bytes, G, N, w));
  hipStream_t st = ctx->stream;
  if (!d_mask) {
    if (nnz > 0) hipLaunchKernelGGL(k_od_scale, dim3(gficf_grid_1d(nnz)), dim3(256), 0, st, G, nnz, d_rowidx, d_x, d_scale, d_out_x, w.status);
    GFICF_HIP_CHECK(hipGetLastError());
    return GFICF_OK;
  }
  if (!d_out_colptr || !d_nsel || (nnz > 0 && !d_out_rowidx)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  if (N > (int64_t)INT32_MAX / 64) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "N = %lld: one wave per column", (long long)N);
  hipLaunchKernelGGL(k_od_newid, dim3(1), dim3(256), 0, st, G, d_mask, w.newid, d_nsel);
  if (N > 0) hipLaunchKernelGGL(k_od_count, dim3(od_waves(N)), dim3(256), 0, st, G, N, nnz, d_colptr, d_rowidx, d_mask, w.cnt, w.status);
  hipLaunchKernelGGL(k_od_colscan, dim3(1), dim3(256), 0, st, N, (const int64_t*)w.cnt, d_out_colptr);
  if (N > 0 && nnz > 0)
    hipLaunchKernelGGL(k_od_write, dim3(od_waves(N)), dim3(256), 0, st, G, N, nnz, d_colptr, d_rowidx, d_x, d_mask, (const int32_t*)w.newid, d_scale,
                       (const int64_t*)d_out_colptr, nnz, d_out_rowidx, d_out_x, w.status);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int gficf_od_sync(gficf_ctx* ctx, const void* ws) {
  uint32_t st;
  const int rc = gficf_addon_read_status(ctx, ws, &st);
  if (rc) return rc;
  if (st) GFICF_HIP_CHECK(hipMemset(const_cast<void*>(ws), 0, sizeof(uint32_t)));
  if (st & OD_ST_CSC) GFICF_FAIL(GFICF_ERR_BAD_CSC, "a row index or a column pointer of the matrix is out of range");
  if (st & OD_ST_ITER) GFICF_FAIL(GFICF_ERR_BAD_VALUE, "a log p-value or an adjusted variance did not converge within its iteration cap");
  return GFICF_OK;
}

int gficf_od_from_moments_host(gficf_ctx* ctx, int64_t G, int64_t N, const double* m, const double* var, const int32_t* nobs, int32_t gam_k,
                               int32_t min_gene_cells, double min_adjusted_variance, double max_adjusted_variance, double sp, double* v, int32_t* valid,
                               double* fit, double* res, double* lp, double* lpa, double* qv, double* gsf, double* info) {
  GFICF_CTX_ENTER(ctx);
  if (!od_sizes_ok(G, N) || N < 2) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "G = %lld, N = %lld: at least one gene and two cells", (long long)G, (long long)N);
  if (!m || !var || !nobs) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  GFICF_RC(od_check_k(gam_k));
  const size_t wsb = gficf_od_workspace_bytes(G, 0), g = (size_t)G;
  gficf_host_io io{ctx, "gficf_od_from_moments_host"};
  gficf_carver cv;
  double *d_m, *d_var, *d_out; int32_t* d_nobs; char* d_ws;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    d_m = cv.take<double>(g); d_var = cv.take<double>(g); d_nobs = cv.take<int32_t>(g); d_out = cv.take<double>(8 * g); d_ws = cv.take<char>(wsb);
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_STAGE0);
  }
  io.up(d_m, m, sizeof(double) * g);
  io.up(d_var, var, sizeof(double) * g);
  io.up(d_nobs, nobs, sizeof(int32_t) * g);
  if (!io.ok()) return io.drain(GFICF_OK);
  const OdOut o{v, fit, res, lp, lpa, qv, gsf, info, valid};
  return od_run(ctx, io, d_ws, wsb, G, N, d_m, d_var, d_nobs, gam_k, min_gene_cells, min_adjusted_variance, max_adjusted_variance, sp, d_out, o);
}

int gficf_od_host(gficf_ctx* ctx, int64_t G, int64_t N, const void* colptr, int colptr_is_i64, const int32_t* rowidx, const double* x, const double* m,
                  int32_t gam_k, int32_t min_gene_cells, double min_adjusted_variance, double max_adjusted_variance, double sp, double* var, int32_t* nobs,
                  double* v, int32_t* valid, double* fit, double* res, double* lp, double* lpa, double* qv, double* gsf, double* info) {
  GFICF_CTX_ENTER(ctx);
  if (!od_sizes_ok(G, N) || N < 2) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "G = %lld, N = %lld: at least one gene and two cells", (long long)G, (long long)N);
  if (!colptr || !m) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  GFICF_RC(od_check_k(gam_k));
  std::vector<int64_t> cp;
  int64_t nnz = 0;
  GFICF_RC(gficf_host_colptr(colptr, colptr_is_i64, N, "colptr", cp, &nnz));
  if (nnz > 0 && (!rowidx || !x)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  const size_t hvb = gficf_hvg_workspace_bytes(G, N, nnz, 0);
  if (hvb == 0) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "G = %lld, N = %lld, nnz = %lld: beyond what the sort and the transpose take", (long long)G, (long long)N, (long long)nnz);
  const size_t wsb = gficf_od_workspace_bytes(G, 0), g = (size_t)G, ne = (size_t)(nnz > 0 ? nnz : 1);
  gficf_host_io io{ctx, "gficf_od_host"};
  gficf_carver cv;
  int64_t* d_cp; int32_t *d_row, *d_nobs, *d_hvalid; double *d_x, *d_m, *d_mean, *d_sd, *d_var, *d_lx, *d_ly, *d_out; char *d_ws, *d_hws;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    d_cp = cv.take<int64_t>((size_t)N + 1); d_row = cv.take<int32_t>(ne); d_x = cv.take<double>(ne); d_m = cv.take<double>(g);
    d_mean = cv.take<double>(g); d_sd = cv.take<double>(g); d_var = cv.take<double>(g); d_lx = cv.take<double>(g); d_ly = cv.take<double>(g);
    d_nobs = cv.take<int32_t>(g); d_hvalid = cv.take<int32_t>(g); d_out = cv.take<double>(8 * g); d_ws = cv.take<char>(wsb); d_hws = cv.take<char>(hvb);
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_STAGE0);
  }
  io.up(d_cp, cp.data(), sizeof(int64_t) * ((size_t)N + 1));
  io.up(d_row, rowidx, sizeof(int32_t) * (size_t)nnz);
  io.up(d_x, x, sizeof(double) * (size_t)nnz);
  io.up(d_m, m, sizeof(double) * g);
  if (!io.ok()) return io.drain(GFICF_OK);
  int rc = gficf_hvg_moments_device(ctx, G, N, d_cp, d_row, d_x, nnz, d_hws, hvb, d_mean, d_sd, d_var, d_nobs, d_lx, d_ly, d_hvalid);
  if (rc) return io.drain(rc);
  if (var) io.down(var, d_var, sizeof(double) * g);
  if (nobs) io.down(nobs, d_nobs, sizeof(int32_t) * g);
  if (!io.ok()) return io.drain(GFICF_OK);
  rc = gficf_hvg_sync(ctx, d_hws);                         // the moments are on the host, the matrix is checked
  if (rc) return rc;
  const OdOut o{v, fit, res, lp, lpa, qv, gsf, info, valid};
  return od_run(ctx, io, d_ws, wsb, G, N, d_m, d_var, d_nobs, gam_k, min_gene_cells, min_adjusted_variance, max_adjusted_variance, sp, d_out, o);
}

int gficf_od_select_scale_host(gficf_ctx* ctx, int64_t G, int64_t N, const void* colptr, int colptr_is_i64, const int32_t* rowidx, const double* x,
                               const int32_t* mask, const double* scale, int64_t* out_colptr, int32_t* out_rowidx, double* out_x, int32_t* out_nsel) {
  GFICF_CTX_ENTER(ctx);
  if (!od_sizes_ok(G, N)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "G = %lld, N = %lld: a size is out of range", (long long)G, (long long)N);
  if (!colptr) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  std::vector<int64_t> cp;
  int64_t nnz = 0;
  GFICF_RC(gficf_host_colptr(colptr, colptr_is_i64, N, "colptr", cp, &nnz));
  if (nnz > 0 && (!rowidx || !x || !out_x)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  if (mask) {
    if (!out_colptr || !out_nsel || (nnz > 0 && !out_rowidx)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
    int64_t sel = 0;
    for (int64_t i = 0; i < G; ++i) sel += mask[i] != 0;
    if (sel == 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "no row is selected: there is nothing to decompose");
  }
  const size_t wsb = gficf_od_workspace_bytes(G, N), g = (size_t)G, ne = (size_t)(nnz > 0 ? nnz : 1);
  gficf_host_io io{ctx, "gficf_od_select_scale_host"};
  gficf_carver cv;
  int64_t *d_cp, *d_ocp; int32_t *d_row, *d_mask, *d_orow, *d_nsel; double *d_x, *d_scale, *d_ox; char* d_ws;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    d_cp = cv.take<int64_t>((size_t)N + 1); d_ocp = cv.take<int64_t>((size_t)N + 1); d_row = cv.take<int32_t>(ne); d_orow = cv.take<int32_t>(ne);
    d_x = cv.take<double>(ne); d_ox = cv.take<double>(ne); d_mask = cv.take<int32_t>(g); d_scale = cv.take<double>(g); d_nsel = cv.take<int32_t>(1);
    d_ws = cv.take<char>(wsb);
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_STAGE0);
  }
  io.up(d_cp, cp.data(), sizeof(int64_t) * ((size_t)N + 1));
  io.up(d_row, rowidx, sizeof(int32_t) * (size_t)nnz);
  io.up(d_x, x, sizeof(double) * (size_t)nnz);
  if (mask) io.up(d_mask, mask, sizeof(int32_t) * g);
  if (scale) io.up(d_scale, scale, sizeof(double) * g);
  if (io.ok()) io.e = hipMemsetAsync(d_ws, 0, sizeof(uint32_t), ctx->stream);
  if (!io.ok()) return io.drain(GFICF_OK);
  int rc = gficf_od_select_scale_device(ctx, G, N, d_cp, d_row, d_x, nnz, mask ? d_mask : nullptr, scale ? d_scale : nullptr, d_ws, wsb, d_ocp, d_orow, d_ox,
                                        d_nsel);
  if (rc) return io.drain(rc);
  if (mask) {
    io.down(out_colptr, d_ocp, sizeof(int64_t) * ((size_t)N + 1));
    io.down(out_rowidx, d_orow, sizeof(int32_t) * (size_t)nnz);
    io.down(out_nsel, d_nsel, sizeof(int32_t));
  }
  io.down(out_x, d_ox, sizeof(double) * (size_t)nnz);
  if (!io.ok()) return io.drain(GFICF_OK);
  return gficf_od_sync(ctx, d_ws);
}

}  // extern "C"
