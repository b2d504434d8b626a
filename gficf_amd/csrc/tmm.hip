// tmm.hip — edgeR's TMM library-size factors and counts per million from the sparse count matrix: the normalize = TRUE branch of
// gficf() and normCounts() (reference R/gficf.R:43-47) for all cells at once.  Built into libgficf_tmm.so, which links
// libgficf_hip.so and uses its context, pool and error plumbing (include/gficf_tmm.h states the contract, the tie rule first).
//
// Nothing is densified.  The zeros of a column are one group: the quantile of stage 1 needs the column's positive values in
// order and the number of zeros in front of them; the common entries of stage 2 are found through a dense table of the one
// reference column (8 B per gene: it stays in L2).  A cell's two rank keys, q = obs / ref and s = obs * ref, are positive
// doubles and order as their bit patterns: two u64 lists sorted in LDS, an entry's average rank two binary searches in each.
// Launches, all on the context's stream:
//   k_tm_rows         the rows that hold a count (G'), every value and row index checked
//   k_tm_gp           G', one workgroup
//   k_tm_stats        one workgroup per cell: lib, sq, its positive values sorted in LDS (or selected by counting), f75
//   k_tm_ref          the reference column scattered into the dense table
//   k_tm_factors      one workgroup per cell: keys into LDS, bitonic sort, ranks, trim, the two folded sums, 2^f;
//                     a cell with more common entries than the LDS lists hold is put on a list instead.  Twice where a
//                     cell may be longer than 2 048: short lists for all cells, then the full capacity for the listed ones
//   k_tm_factors_big  one workgroup per listed cell: keys into global workspace, ranks by counting over them in LDS tiles
//   k_tm_cpm          one workgroup per cell: x / (1e-6 * (lib * f))
#include <algorithm>
#include <cmath>
#include <vector>

#include "addon_status.h"
#include "block_ops.h"
#include "common.h"
#include "gficf_tmm.h"

namespace {

typedef unsigned long long u64;

constexpr uint32_t TM_ST_VALUE = 1u;                     // a negative, NaN or infinite value
constexpr uint32_t TM_ST_INDEX = 2u;                     // a row outside [0, G), or a row twice in a column
constexpr uint32_t TM_ST_PTR = 4u;                       // offsets that decrease or leave [0, nnz]
constexpr int32_t TM_TIER1 = 2048;                       // keys per LDS list of the factor kernel's first tier
constexpr uint32_t TM_ST_BIG = 8u;                       // more cells or entries beyond the LDS capacity than announced

__device__ inline int64_t tm_at(const void* p, int is64, int64_t i) {
  return is64 ? ((const int64_t*)p)[i] : (int64_t)((const int32_t*)p)[i];
}

// the average rank of v among the ascending a[0 .. n), v one of them: #less + (#equal + 1) / 2.  The keys are the bits of
// doubles that are not negative (the sign bit is clear), so v + 1 does not wrap: the first key above v is the first not below it.
__device__ inline double tm_rank(const u64* a, int n, u64 v) {
  const int less = gficf_lower_bound(a, n, v);
  const int equal = gficf_lower_bound(a + less, n - less, v + 1);
  return (double)less + (double)(equal + 1) / 2.0;
}

__global__ __launch_bounds__(256) void k_tm_rows(int64_t G, int64_t nnz, const int32_t* __restrict__ row, const double* __restrict__ x,
                                                 int32_t* __restrict__ flag, uint32_t* __restrict__ status) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * 256) {
    const double v = x[e];
    const int32_t g = row[e];
    if (!(v >= 0.0) || !isfinite(v)) atomicOr(status, TM_ST_VALUE);
    if (g < 0 || g >= G) { atomicOr(status, TM_ST_INDEX); continue; }
    if (v > 0.0) flag[g] = 1;                              // every writer stores the same value
  }
}

__global__ __launch_bounds__(256) void k_tm_gp(int64_t G, const int32_t* __restrict__ flag, int32_t* __restrict__ gp, int32_t* __restrict__ gp_out) {
  __shared__ int32_t s_c;
  if (threadIdx.x == 0) s_c = 0;
  __syncthreads();
  int32_t cnt = 0;
  for (int64_t g = threadIdx.x; g < G; g += 256) cnt += flag[g] != 0 ? 1 : 0;
  atomicAdd(&s_c, cnt);
  __syncthreads();
  if (threadIdx.x == 0) { gp[0] = s_c; gp_out[0] = s_c; }
}

// One workgroup per cell.  keys: the cell's positive values (dynamic LDS, npad >= cap entries).
__global__ __launch_bounds__(256) void k_tm_stats(int64_t N, const void* __restrict__ colptr, int is64, const double* __restrict__ x, int64_t nnz, int32_t cap,
                                                  const int32_t* __restrict__ gp, double* __restrict__ lib, double* __restrict__ sq,
                                                  double* __restrict__ f75, double* __restrict__ ostat, uint32_t* __restrict__ status) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char tm_lds[];
  u64* keys = (u64*)tm_lds;
  __shared__ double s_fold[256];
  __shared__ double s_res[2];
  __shared__ int32_t s_n;
  const int t = threadIdx.x;
  const int64_t c = blockIdx.x, beg = tm_at(colptr, is64, c), end = tm_at(colptr, is64, c + 1);
  if (beg < 0 || end < beg || end > nnz) {
    if (t == 0) { atomicOr(status, TM_ST_PTR); lib[c] = 0.0; sq[c] = 0.0; f75[c] = 0.0; ostat[c] = 0.0; ostat[N + c] = 0.0; }
    return;
  }
  if (t == 0) { s_n = 0; s_res[0] = 0.0; s_res[1] = 0.0; }
  __syncthreads();
  double a = 0.0, b = 0.0;
  for (int64_t e = beg + t; e < end; e += 256) {
    const double v = x[e];
    if (v > 0.0 && isfinite(v)) {                          // anything else is flagged by k_tm_rows
      a += v;
      b += sqrt(v);
      const int i = atomicAdd(&s_n, 1);                    // any slot: the sort fixes the order
      if (i < cap) keys[i] = (u64)__double_as_longlong(v);
    }
  }
  const double L = gficf_block_sum_f64(a, s_fold), S = gficf_block_sum_f64(b, s_fold);
  const int64_t npos = s_n, Gp = gp[0];
  double q = 0.0, xlo = 0.0, xhi = 0.0;
  if (Gp > 0) {
    const double idx = (double)(Gp - 1) * 0.75, lo = floor(idx), hi = ceil(idx);
    const int64_t z = Gp - npos, klo = (int64_t)lo - z, khi = (int64_t)hi - z;
    if (khi >= npos) {                                     // more positive values than rows that hold one: a row twice
      if (t == 0) atomicOr(status, TM_ST_INDEX);
    } else if (khi >= 0) {
      if (npos <= cap) {
        int np2 = 1;
        while (np2 < npos) np2 <<= 1;
        for (int i = (int)npos + t; i < np2; i += 256) keys[i] = ~0ull;
        __syncthreads();
        gficf_lds_sort_u64(keys, np2);
        if (t == 0) {
          s_res[0] = klo >= 0 ? __longlong_as_double((long long)keys[klo]) : 0.0;
          s_res[1] = __longlong_as_double((long long)keys[khi]);
        }
      } else {                                             // select by counting: the value with #less <= k < #less + #equal
        for (int64_t e = beg + t; e < end; e += 256) {
          const double v = x[e];
          if (!(v > 0.0)) continue;
          int64_t less = 0, eq = 0;
          for (int64_t j = beg; j < end; ++j) {
            const double w = x[j];
            if (w > 0.0) { less += w < v ? 1 : 0; eq += w == v ? 1 : 0; }
          }
          if (klo >= less && klo < less + eq) s_res[0] = v;   // every writer stores the same value
          if (khi >= less && khi < less + eq) s_res[1] = v;
        }
      }
      __syncthreads();
      xlo = s_res[0];
      xhi = s_res[1];
    }
    q = xlo;
    const double h = idx - lo;
    if (idx > lo && xhi != q) q = (1.0 - h) * q + h * xhi;
  }
  if (t == 0) {
    lib[c] = L;
    sq[c] = S;
    f75[c] = L > 0.0 ? q / L : 0.0;
    ostat[c] = xlo;
    ostat[N + c] = xhi;
  }
}

__global__ __launch_bounds__(256) void k_tm_ref(int64_t G, const void* __restrict__ colptr, int is64, int64_t ref_col, int64_t nnz,
                                                const int32_t* __restrict__ row, const double* __restrict__ x, double* __restrict__ ref) {
  const int64_t beg = tm_at(colptr, is64, ref_col), end = tm_at(colptr, is64, ref_col + 1);
  if (beg < 0 || end < beg || end > nnz) return;           // flagged by k_tm_factors, whose grid holds the column
  for (int64_t e = beg + (int64_t)blockIdx.x * 256 + threadIdx.x; e < end; e += (int64_t)gridDim.x * 256) {
    const int32_t g = row[e];
    const double v = x[e];
    if (g >= 0 && g < G && v > 0.0 && isfinite(v)) ref[g] = v;
  }
}

struct TmTrim {
  double nO, nR, loL, hiL, loS, hiS;
  int dw;
};

// loL .. hiS of the header for a cell of n common entries
__device__ inline void tm_bounds(int n, double lt, double st, TmTrim& b) {
#pragma clang fp contract(off)
  b.loL = floor((double)n * lt) + 1.0;
  b.hiL = (double)n + 1.0 - b.loL;
  b.loS = floor((double)n * st) + 1.0;
  b.hiS = (double)n + 1.0 - b.loS;
}

__device__ inline double tm_logr(double obs, double r, double nO, double nR) {
#pragma clang fp contract(off)
  return log2((obs / nO) / (r / nR));
}

// the term of one common entry with the average ranks rq, rs into thread t's partial sums
__device__ inline void tm_term(double obs, double r, double rq, double rs, const TmTrim& b, double& num, double& den, int& kept) {
#pragma clang fp contract(off)
  if (!(rq >= b.loL && rq <= b.hiL && rs >= b.loS && rs <= b.hiS)) return;
  ++kept;
  const double logR = tm_logr(obs, r, b.nO, b.nR);
  if (b.dw) {
    const double v = (b.nO - obs) / b.nO / obs + (b.nR - r) / b.nR / r;
    const double p = logR / v, w = 1.0 / v;
    if (p == p) num += p;                                  // na.rm, each sum on its own
    if (w == w) den += w;
  } else if (logR == logR) {
    num += logR;
    den += 1.0;
  }
}

// the folds and the factor; s_kept is a zeroed LDS counter
__device__ inline void tm_finish(int64_t c, int n, double num, double den, int kept, double mx, double* s_fold, int32_t* s_kept,
                                 double* __restrict__ factor, int32_t* __restrict__ n_out, int32_t* __restrict__ kept_out) {
#pragma clang fp contract(off)
  const double A = gficf_block_sum_f64(num, s_fold), B = gficf_block_sum_f64(den, s_fold), M = gficf_block_max_f64(mx, s_fold);
  atomicAdd(s_kept, kept);
  __syncthreads();
  if (threadIdx.x == 0) {
    const double f = A / B;
    double fac = exp2(f);
    if (f != f || M < 1e-6) fac = 1.0;
    factor[c] = fac;
    n_out[c] = n;
    kept_out[c] = *s_kept;
  }
}

// what the factor kernel is given besides the matrix
struct TmArgs {
  int64_t G, nnz, ref_col, over_cap;
  const double *ref, *lib;
  double lt, st;
  int dw;
  int32_t cap, npad;
  uint32_t* over_cnt;                                      // the cells with more common entries than cap: counted and listed for the next tier
  int32_t* over_list;
  double* factor;
  int32_t *n_out, *kept_out;
  uint32_t* status;
};

// The whole workgroup on cell c.  Kq, Ks: the keys of its common entries (dynamic LDS, npad >= cap entries each).
__device__ inline void tm_cell(int64_t c, const void* __restrict__ colptr, int is64, const int32_t* __restrict__ row, const double* __restrict__ x,
                               const TmArgs& A, u64* Kq, u64* Ks, double* s_fold, int32_t* s_cnt) {
#pragma clang fp contract(off)
  const int64_t G = A.G, nnz = A.nnz;
  const double* __restrict__ ref = A.ref;
  const int32_t cap = A.cap;
  double* factor = A.factor;
  int32_t *n_out = A.n_out, *kept_out = A.kept_out;
  uint32_t* status = A.status;
  int32_t& s_n = s_cnt[0];
  int32_t& s_kept = s_cnt[1];
  const int t = threadIdx.x;
  const int64_t beg = tm_at(colptr, is64, c), end = tm_at(colptr, is64, c + 1);
  if (beg < 0 || end < beg || end > nnz) {
    if (t == 0) { atomicOr(status, TM_ST_PTR); factor[c] = 1.0; n_out[c] = 0; kept_out[c] = 0; }
    return;
  }
  __syncthreads();                                         // the previous cell of this workgroup is done with the LDS
  if (t == 0) { s_n = 0; s_kept = 0; }
  __syncthreads();
  TmTrim b;
  b.nO = A.lib[c];
  b.nR = A.lib[A.ref_col];
  b.dw = A.dw;
  double mx = 0.0;
  for (int64_t e = beg + t; e < end; e += 256) {
    const int32_t g = row[e];
    if (g < 0 || g >= G) { atomicOr(status, TM_ST_INDEX); continue; }
    const double obs = x[e], r = ref[g];
    if (!(obs > 0.0) || !(r > 0.0) || !isfinite(obs)) continue;
    mx = fmax(mx, fabs(tm_logr(obs, r, b.nO, b.nR)));
    const int i = atomicAdd(&s_n, 1);                      // any slot: the sorts fix the order, equal keys are the same bits
    if (i < cap) {
      Kq[i] = (u64)__double_as_longlong(obs / r);
      Ks[i] = (u64)__double_as_longlong(obs * r);
    }
  }
  __syncthreads();
  const int n = s_n;
  if (n > cap) {                                           // ranked by the next tier: longer LDS lists, or k_tm_factors_big
    if (t == 0) {
      factor[c] = 1.0; n_out[c] = n; kept_out[c] = 0;
      const uint32_t i = atomicAdd(A.over_cnt, 1u);
      if ((int64_t)i < A.over_cap) A.over_list[i] = (int32_t)c; else atomicOr(status, TM_ST_BIG);
    }
    return;
  }
  int np2 = 1;
  while (np2 < n) np2 <<= 1;
  for (int i = n + t; i < np2; i += 256) { Kq[i] = ~0ull; Ks[i] = ~0ull; }
  __syncthreads();
  gficf_lds_sort_u64(Kq, np2);
  gficf_lds_sort_u64(Ks, np2);
  tm_bounds(n, A.lt, A.st, b);
  double num = 0.0, den = 0.0;
  int kept = 0;
  for (int64_t e = beg + t; e < end; e += 256) {
    const int32_t g = row[e];
    if (g < 0 || g >= G) continue;
    const double obs = x[e], r = ref[g];
    if (!(obs > 0.0) || !(r > 0.0) || !isfinite(obs)) continue;
    const double rq = tm_rank(Kq, n, (u64)__double_as_longlong(obs / r)), rs = tm_rank(Ks, n, (u64)__double_as_longlong(obs * r));
    tm_term(obs, r, rq, rs, b, num, den, kept);
  }
  tm_finish(c, n, num, den, kept, mx, s_fold, &s_kept, factor, n_out, kept_out);
}

// LIST false: one workgroup per cell, LDS lists short enough for several workgroups to share a CU.  LIST true: the cells the
// first tier listed, dealt to the workgroups in turn, LDS lists of the full capacity.
template <bool LIST>
__global__ __launch_bounds__(256) void k_tm_factors(const void* __restrict__ colptr, int is64, const int32_t* __restrict__ row, const double* __restrict__ x,
                                                    const uint32_t* __restrict__ list_cnt, const int32_t* __restrict__ list, int64_t list_cap, TmArgs A) {
  extern __shared__ __align__(16) unsigned char tm_lds[];
  u64* Kq = (u64*)tm_lds;
  u64* Ks = Kq + A.npad;
  __shared__ double s_fold[256];
  __shared__ int32_t s_cnt[2];
  if (!LIST) {
    tm_cell(blockIdx.x, colptr, is64, row, x, A, Kq, Ks, s_fold, s_cnt);
  } else {
    const int64_t m = (int64_t)*list_cnt < list_cap ? (int64_t)*list_cnt : list_cap;
    for (int64_t i = blockIdx.x; i < m; i += gridDim.x) tm_cell(list[i], colptr, is64, row, x, A, Kq, Ks, s_fold, s_cnt);
  }
}

// One workgroup per cell of the list.  The keys of all its stored entries go to the workspace at the entry's place in the
// column (0: not a common entry), then every entry is ranked by counting over them, staged through LDS in tiles of 256.
__global__ __launch_bounds__(256) void k_tm_factors_big(int64_t G, const void* __restrict__ colptr, int is64, const int32_t* __restrict__ row,
                                                        const double* __restrict__ x, int64_t ref_col, const double* __restrict__ ref,
                                                        const double* __restrict__ lib, double lt, double st, int dw,
                                                        const uint32_t* __restrict__ big_cnt, const int32_t* __restrict__ big_list, u64* __restrict__ cursor,
                                                        u64* __restrict__ wq, u64* __restrict__ wsk, int64_t big_entries, double* __restrict__ factor,
                                                        int32_t* __restrict__ n_out, int32_t* __restrict__ kept_out, uint32_t* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ double s_fold[256];
  __shared__ u64 s_q[256], s_s[256];
  __shared__ u64 s_off;
  __shared__ int32_t s_n, s_kept;
  const int t = threadIdx.x;
  if (blockIdx.x >= *big_cnt) return;
  const int64_t c = big_list[blockIdx.x], beg = tm_at(colptr, is64, c), end = tm_at(colptr, is64, c + 1), nz = end - beg;   // checked by k_tm_factors
  if (t == 0) { s_off = atomicAdd(cursor, (u64)nz); s_n = 0; s_kept = 0; }
  __syncthreads();
  const int64_t off = (int64_t)s_off;
  if (off + nz > big_entries) {
    if (t == 0) atomicOr(status, TM_ST_BIG);
    return;
  }
  u64* Kq = wq + off;
  u64* Ks = wsk + off;
  TmTrim b;
  b.nO = lib[c];
  b.nR = lib[ref_col];
  b.dw = dw;
  double mx = 0.0;
  int cnt = 0;
  for (int64_t i = t; i < nz; i += 256) {
    const int32_t g = row[beg + i];
    const double obs = x[beg + i], r = (g >= 0 && g < G) ? ref[g] : 0.0;
    u64 kq = 0ull, ks = 0ull;
    if (obs > 0.0 && r > 0.0 && isfinite(obs)) {
      mx = fmax(mx, fabs(tm_logr(obs, r, b.nO, b.nR)));
      kq = (u64)__double_as_longlong(obs / r);
      ks = (u64)__double_as_longlong(obs * r);
      ++cnt;
    }
    Kq[i] = kq;
    Ks[i] = ks;
  }
  atomicAdd(&s_n, cnt);
  __syncthreads();                                         // the keys are written, s_n is whole
  const int n = s_n;
  tm_bounds(n, lt, st, b);
  double num = 0.0, den = 0.0;
  int kept = 0;
  for (int64_t i0 = 0; i0 < nz; i0 += 256) {
    const int64_t i = i0 + t;
    const u64 kq = i < nz ? Kq[i] : 0ull, ks = i < nz ? Ks[i] : 0ull;
    int lq = 0, eq = 0, ls = 0, es = 0;
    for (int64_t j0 = 0; j0 < nz; j0 += 256) {
      __syncthreads();
      if (j0 + t < nz) { s_q[t] = Kq[j0 + t]; s_s[t] = Ks[j0 + t]; }
      __syncthreads();
      const int len = (int)(nz - j0 < 256 ? nz - j0 : 256);
      if (kq != 0ull)
        for (int j = 0; j < len; ++j) {
          const u64 a = s_q[j], d = s_s[j];
          if (a != 0ull) {
            lq += a < kq ? 1 : 0; eq += a == kq ? 1 : 0;
            ls += d < ks ? 1 : 0; es += d == ks ? 1 : 0;
          }
        }
    }
    if (kq != 0ull) {
      const double rq = (double)lq + (double)(eq + 1) / 2.0, rs = (double)ls + (double)(es + 1) / 2.0;
      tm_term(x[beg + i], ref[row[beg + i]], rq, rs, b, num, den, kept);
    }
  }
  tm_finish(c, n, num, den, kept, mx, s_fold, &s_kept, factor, n_out, kept_out);
}

__global__ __launch_bounds__(256) void k_tm_cpm(const void* __restrict__ colptr, int is64, const double* __restrict__ x, int64_t nnz,
                                                const double* __restrict__ lib, const double* __restrict__ factor, double* __restrict__ out,
                                                uint32_t* __restrict__ status) {
#pragma clang fp contract(off)
  const int64_t c = blockIdx.x, beg = tm_at(colptr, is64, c), end = tm_at(colptr, is64, c + 1);
  if (beg < 0 || end < beg || end > nnz) {
    if (threadIdx.x == 0) atomicOr(status, TM_ST_PTR);
    return;
  }
  const double d = 1e-6 * (lib[c] * factor[c]);
  for (int64_t e = beg + threadIdx.x; e < end; e += 256) out[e] = x[e] / d;
}

// ------------------------------------------------------- workspace
struct TmWs {
  uint32_t* status;
  uint32_t *big_cnt, *mid_cnt;
  u64* cursor;
  int32_t *gp, *flag, *mid_list, *big_list;
  double* ref;
  u64 *wq, *wsk;
};

static size_t tm_carve(char* base, int64_t G, int64_t N, int64_t big_cells, int64_t big_entries, TmWs& w) {
  gficf_carver cv;
  cv.base = base;
  w.status = cv.take<uint32_t>(1);
  w.big_cnt = cv.take<uint32_t>(1);
  w.mid_cnt = cv.take<uint32_t>(1);
  w.cursor = cv.take<u64>(1);
  w.gp = cv.take<int32_t>(1);
  w.flag = cv.take<int32_t>((size_t)G);
  w.ref = cv.take<double>((size_t)G);
  w.mid_list = cv.take<int32_t>((size_t)N);
  w.big_list = cv.take<int32_t>((size_t)std::max<int64_t>(big_cells, 1));
  w.wq = cv.take<u64>((size_t)std::max<int64_t>(big_entries, 1));
  w.wsk = cv.take<u64>((size_t)std::max<int64_t>(big_entries, 1));
  return cv.total();
}

static int tm_check_sizes(int64_t G, int64_t N, int64_t nnz, int64_t max_cell_nz, int64_t max_lds_n) {
  if (G < 1 || N < 1 || nnz < 0 || max_cell_nz < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "G = %lld, N = %lld, nnz = %lld, max_cell_nz = %lld: a size is out of range", (long long)G, (long long)N, (long long)nnz, (long long)max_cell_nz);
  if (G > INT32_MAX || N > INT32_MAX) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "more than 2^31 - 1 genes or cells");
  if (max_cell_nz > INT32_MAX) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "a cell with more than 2^31 - 1 stored entries");
  if (max_lds_n < 0 || max_lds_n > GFICF_TMM_LDS_N) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "max_lds_n = %lld: 0 or 1 .. %d", (long long)max_lds_n, GFICF_TMM_LDS_N);
  return GFICF_OK;
}

static int tm_workspace(void* ws, size_t ws_bytes, int64_t G, int64_t N, int64_t big_cells, int64_t big_entries, TmWs& w) {
  if (!ws) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL workspace");
  if (big_cells < 0 || big_entries < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "big_cells = %lld, big_entries = %lld", (long long)big_cells, (long long)big_entries);
  return gficf_addon_carve(ws, ws_bytes, [&](char* base) { return tm_carve(base, G, N, big_cells, big_entries, w); });
}

// the LDS list length (a power of two, at least 64) and the capacity the kernels keep to, from the caller's bounds
static void tm_lds_shape(int64_t max_cell_nz, int64_t max_lds_n, int32_t* cap, int32_t* npad) {
  const int64_t lim = max_lds_n > 0 ? max_lds_n : GFICF_TMM_LDS_N;
  int64_t np = 64;
  while (np < std::min(max_cell_nz, lim)) np <<= 1;
  *npad = (int32_t)np;
  *cap = (int32_t)std::min(lim, np);
}

}  // namespace

extern "C" {

int gficf_tmm_abi_version(void) { return GFICF_TMM_ABI_VERSION; }

size_t gficf_tmm_workspace_bytes(int64_t G, int64_t N, int64_t big_cells, int64_t big_entries) {
  if (G < 1 || N < 1 || G > INT32_MAX || N > INT32_MAX || big_cells < 0 || big_entries < 0) return 0;
  TmWs w;
  return tm_carve(nullptr, G, N, big_cells, big_entries, w);
}

int gficf_tmm_stats_device(gficf_ctx* ctx, int64_t G, int64_t N, const void* d_colptr, int colptr_is_i64, const int32_t* d_rowidx, const double* d_x,
                           int64_t nnz, int64_t max_cell_nz, int64_t max_lds_n, void* ws, size_t ws_bytes, double* d_lib, double* d_sq,
                           double* d_f75, double* d_ostat, int32_t* d_gprime) {
  GFICF_CTX_ENTER(ctx);
  int rc = tm_check_sizes(G, N, nnz, max_cell_nz, max_lds_n);
  if (rc) return rc;
  if (!d_colptr || !d_lib || !d_sq || !d_f75 || !d_ostat || !d_gprime || (nnz > 0 && (!d_rowidx || !d_x))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  TmWs w;
  rc = tm_workspace(ws, ws_bytes, G, N, 0, 0, w);
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  GFICF_HIP_CHECK(hipMemsetAsync(w.status, 0, sizeof(uint32_t), st));
  GFICF_HIP_CHECK(hipMemsetAsync(w.flag, 0, sizeof(int32_t) * (size_t)G, st));
  hipLaunchKernelGGL(k_tm_rows, dim3(gficf_grid_1d(nnz)), dim3(256), 0, st, G, nnz, d_rowidx, d_x, w.flag, w.status);
  hipLaunchKernelGGL(k_tm_gp, dim3(1), dim3(256), 0, st, G, (const int32_t*)w.flag, w.gp, d_gprime);
  GFICF_HIP_CHECK(hipGetLastError());
  int32_t cap, npad;
  tm_lds_shape(max_cell_nz, max_lds_n, &cap, &npad);
  const size_t lds = sizeof(u64) * (size_t)npad;
  GFICF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_tm_stats), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_tm_stats, dim3((unsigned)N), dim3(256), lds, st, N, d_colptr, colptr_is_i64, d_x, nnz, cap, (const int32_t*)w.gp, d_lib, d_sq, d_f75,
                     d_ostat, w.status);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int gficf_tmm_factors_device(gficf_ctx* ctx, int64_t G, int64_t N, const void* d_colptr, int colptr_is_i64, const int32_t* d_rowidx, const double* d_x,
                             int64_t nnz, int64_t max_cell_nz, int64_t ref_col, const double* d_lib, double logratio_trim, double sum_trim,
                             int32_t do_weighting, int64_t max_lds_n, int64_t big_cells, int64_t big_entries, int32_t fresh, void* ws,
                             size_t ws_bytes, double* d_factor, int32_t* d_n, int32_t* d_kept) {
  GFICF_CTX_ENTER(ctx);
  int rc = tm_check_sizes(G, N, nnz, max_cell_nz, max_lds_n);
  if (rc) return rc;
  if (ref_col < 0 || ref_col >= N) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "ref_col = %lld outside [0, %lld)", (long long)ref_col, (long long)N);
  if (!(logratio_trim >= 0.0 && logratio_trim < 0.5) || !(sum_trim >= 0.0 && sum_trim < 0.5))
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "logratioTrim = %g, sumTrim = %g: each must lie in [0, 0.5)", logratio_trim, sum_trim);
  if (big_cells > N) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "big_cells = %lld, but %lld cells", (long long)big_cells, (long long)N);
  if (!d_colptr || !d_lib || !d_factor || !d_n || !d_kept || (nnz > 0 && (!d_rowidx || !d_x))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  TmWs w;
  rc = tm_workspace(ws, ws_bytes, G, N, big_cells, big_entries, w);
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  if (fresh) GFICF_HIP_CHECK(hipMemsetAsync(w.status, 0, sizeof(uint32_t), st));
  GFICF_HIP_CHECK(hipMemsetAsync(w.big_cnt, 0, sizeof(uint32_t), st));
  GFICF_HIP_CHECK(hipMemsetAsync(w.mid_cnt, 0, sizeof(uint32_t), st));
  GFICF_HIP_CHECK(hipMemsetAsync(w.cursor, 0, sizeof(u64), st));
  GFICF_HIP_CHECK(hipMemsetAsync(w.ref, 0, sizeof(double) * (size_t)G, st));
  hipLaunchKernelGGL(k_tm_ref, dim3(gficf_grid_1d(std::min(max_cell_nz, G))), dim3(256), 0, st, G, d_colptr, colptr_is_i64, ref_col, nnz, d_rowidx, d_x, w.ref);
  GFICF_HIP_CHECK(hipGetLastError());
  int32_t cap, npad;
  tm_lds_shape(max_cell_nz, max_lds_n, &cap, &npad);
  // two tiers of LDS lists: every cell first with lists of at most TM_TIER1 keys (32 KiB a workgroup: five share a CU), the
  // few longer ones again with lists of the full capacity (one workgroup a CU), what is longer still by counting
  TmArgs A{G, nnz, ref_col, 0, w.ref, d_lib, logratio_trim, sum_trim, do_weighting ? 1 : 0, 0, 0, nullptr, nullptr, d_factor, d_n, d_kept, w.status};
  const bool two = npad > TM_TIER1;
  A.npad = two ? TM_TIER1 : npad;
  A.cap = std::min(cap, A.npad);
  A.over_cnt = two ? w.mid_cnt : w.big_cnt;
  A.over_list = two ? w.mid_list : w.big_list;
  A.over_cap = two ? N : big_cells;
  hipLaunchKernelGGL(k_tm_factors<false>, dim3((unsigned)N), dim3(256), 2 * sizeof(u64) * (size_t)A.npad, st, d_colptr, colptr_is_i64, d_rowidx, d_x,
                     (const uint32_t*)nullptr, (const int32_t*)nullptr, (int64_t)0, A);
  GFICF_HIP_CHECK(hipGetLastError());
  if (two) {
    A.npad = npad;
    A.cap = cap;
    A.over_cnt = w.big_cnt;
    A.over_list = w.big_list;
    A.over_cap = big_cells;
    const size_t lds = 2 * sizeof(u64) * (size_t)npad;
    GFICF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_tm_factors<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_tm_factors<true>, dim3((unsigned)std::min<int64_t>(N, 4 * (int64_t)ctx->num_cus)), dim3(256), lds, st, d_colptr, colptr_is_i64, d_rowidx,
                       d_x, (const uint32_t*)w.mid_cnt, (const int32_t*)w.mid_list, N, A);
    GFICF_HIP_CHECK(hipGetLastError());
  }
  if (big_cells > 0) {
    hipLaunchKernelGGL(k_tm_factors_big, dim3((unsigned)big_cells), dim3(256), 0, st, G, d_colptr, colptr_is_i64, d_rowidx, d_x, ref_col, (const double*)w.ref,
                       d_lib, logratio_trim, sum_trim, do_weighting ? 1 : 0, (const uint32_t*)w.big_cnt, (const int32_t*)w.big_list, w.cursor, w.wq, w.wsk,
                       big_entries, d_factor, d_n, d_kept, w.status);
    GFICF_HIP_CHECK(hipGetLastError());
  }
  return GFICF_OK;
}

int gficf_tmm_cpm_device(gficf_ctx* ctx, int64_t N, const void* d_colptr, int colptr_is_i64, const double* d_x, int64_t nnz, const double* d_lib,
                         const double* d_factor, void* ws, size_t ws_bytes, double* d_out) {
  GFICF_CTX_ENTER(ctx);
  if (N < 1 || N > INT32_MAX || nnz < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "N = %lld, nnz = %lld: a size is out of range", (long long)N, (long long)nnz);
  if (!d_colptr || !d_lib || !d_factor || !ws || ws_bytes < sizeof(uint32_t) || (nnz > 0 && (!d_x || !d_out))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  hipLaunchKernelGGL(k_tm_cpm, dim3((unsigned)N), dim3(256), 0, ctx->stream, d_colptr, colptr_is_i64, d_x, nnz, d_lib, d_factor, d_out, (uint32_t*)ws);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int gficf_tmm_sync(gficf_ctx* ctx, const void* ws) {
  uint32_t st;
  const int rc = gficf_addon_read_status(ctx, ws, &st);
  if (rc) return rc;
  if (st & TM_ST_PTR) GFICF_FAIL(GFICF_ERR_BAD_CSC, "colptr decreases or leaves [0, nnz]");
  if (st & TM_ST_INDEX) GFICF_FAIL(GFICF_ERR_BAD_CSC, "a row index outside [0, G), or a row twice in a column");
  if (st & TM_ST_VALUE) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "the counts hold a negative, NaN or infinite value");
  if (st & TM_ST_BIG) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "more cells or entries beyond the LDS capacity than big_cells / big_entries announce");
  return GFICF_OK;
}

}  // extern "C"

namespace {

// the exactly rounded sum of v[0 .. n) (Shewchuk's partials, as Python's math.fsum)
static double tm_fsum(const double* v, int64_t n) {
  std::vector<double> p;
  for (int64_t i = 0; i < n; ++i) {
    double x = v[i];
    size_t k = 0;
    for (size_t j = 0; j < p.size(); ++j) {
      double y = p[j];
      if (std::fabs(x) < std::fabs(y)) std::swap(x, y);
      const double hi = x + y, lo = y - (hi - x);
      if (lo != 0.0) p[k++] = lo;
      x = hi;
    }
    p.resize(k);
    p.push_back(x);
  }
  size_t m = p.size();
  double hi = 0.0, lo = 0.0;
  if (m > 0) {
    hi = p[--m];
    while (m > 0) {
      const double x = hi, y = p[--m];
      hi = x + y;
      lo = y - (hi - x);
      if (lo != 0.0) break;
    }
    if (m > 0 && ((lo < 0.0 && p[m - 1] < 0.0) || (lo > 0.0 && p[m - 1] > 0.0))) {   // half-way: round to even needs the next partial
      const double y = lo * 2.0, x = hi + y;
      if (y == x - hi) hi = x;
    }
  }
  return hi;
}

// edgeR's choice of the reference column from stage 1
static int64_t tm_choose_ref(const double* f75, const double* sq, int64_t N) {
  std::vector<double> s(f75, f75 + N);
  std::sort(s.begin(), s.end());
  const double med = (N & 1) ? s[(size_t)(N / 2)] : (s[(size_t)(N / 2 - 1)] + s[(size_t)(N / 2)]) / 2.0;
  int64_t best = 0;
  if (med < 1e-20) {
    for (int64_t c = 1; c < N; ++c)
      if (sq[c] > sq[best]) best = c;
  } else {
    const double mean = tm_fsum(f75, N) / (double)N;
    for (int64_t c = 1; c < N; ++c)
      if (std::fabs(f75[c] - mean) < std::fabs(f75[best] - mean)) best = c;
  }
  return best;
}

}  // namespace

extern "C" {

int gficf_tmm_host(gficf_ctx* ctx, int64_t G, int64_t N, const void* colptr, int colptr_is_i64, const int32_t* rowidx, const double* x, int64_t ref_col,
                   double logratio_trim, double sum_trim, int32_t do_weighting, int64_t max_lds_n, const double* lib_in, const double* factor_in,
                   double* lib, double* sq, double* f75, double* ostat, int32_t* gprime, int64_t* ref_out, double* factor_raw, double* factor,
                   int32_t* n, int32_t* kept, double* cpm) {
  GFICF_CTX_ENTER(ctx);
  if (G < 1 || N < 1) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "G = %lld, N = %lld: a size is out of range", (long long)G, (long long)N);
  if (!colptr) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "colptr is NULL");
  std::vector<int64_t> cp;
  int64_t nnz = 0;
  int rc = gficf_host_colptr(colptr, colptr_is_i64, N, "colptr", cp, &nnz);
  if (rc) return rc;
  const int64_t lim = max_lds_n > 0 ? max_lds_n : GFICF_TMM_LDS_N;
  int64_t max_cell = 0, big_cells = 0, big_entries = 0;
  for (int64_t c = 0; c < N; ++c) {
    const int64_t nz = cp[(size_t)c + 1] - cp[(size_t)c];
    max_cell = std::max(max_cell, nz);
    if (nz > lim) { ++big_cells; big_entries += nz; }
  }
  rc = tm_check_sizes(G, N, nnz, max_cell, max_lds_n);
  if (rc) return rc;
  const bool only_cpm = factor_in != nullptr;
  if (only_cpm ? !cpm : (!lib || !factor || !gprime || !ref_out)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  if (nnz > 0 && (!x || ((!only_cpm || !lib_in) && !rowidx))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  if (!only_cpm && ref_col >= N) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "refColumn = %lld outside [0, %lld)", (long long)ref_col, (long long)N);
  const size_t ne = (size_t)(nnz > 0 ? nnz : 1), wsb = gficf_tmm_workspace_bytes(G, N, big_cells, big_entries);
  gficf_host_io io{ctx, "gficf_tmm_host"};
  gficf_carver cv;
  int64_t* d_cp; int32_t *d_row, *d_gp, *d_n, *d_kept; double *d_x, *d_lib, *d_sq, *d_f75, *d_os, *d_f, *d_out; char* d_ws;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    d_cp = cv.take<int64_t>((size_t)N + 1); d_row = cv.take<int32_t>(ne); d_x = cv.take<double>(ne);
    d_lib = cv.take<double>((size_t)N); d_sq = cv.take<double>((size_t)N); d_f75 = cv.take<double>((size_t)N); d_os = cv.take<double>(2 * (size_t)N);
    d_gp = cv.take<int32_t>(1); d_f = cv.take<double>((size_t)N); d_n = cv.take<int32_t>((size_t)N); d_kept = cv.take<int32_t>((size_t)N);
    d_out = cv.take<double>(cpm ? ne : 1); d_ws = cv.take<char>(wsb);
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_STAGE0);
  }
  io.up(d_cp, cp.data(), sizeof(int64_t) * ((size_t)N + 1));
  io.up(d_x, x, sizeof(double) * (size_t)nnz);
  if (only_cpm) {
    io.up(d_f, factor_in, sizeof(double) * (size_t)N);
    if (lib_in) io.up(d_lib, lib_in, sizeof(double) * (size_t)N);
    else io.up(d_row, rowidx, sizeof(int32_t) * (size_t)nnz);
    if (io.ok()) {
      if (lib_in) io.e = hipMemsetAsync(d_ws, 0, sizeof(uint32_t), ctx->stream);
      else rc = gficf_tmm_stats_device(ctx, G, N, d_cp, 1, d_row, d_x, nnz, max_cell, max_lds_n, d_ws, wsb, d_lib, d_sq, d_f75, d_os, d_gp);   // lib = colSums
      if (io.ok() && !rc) rc = gficf_tmm_cpm_device(ctx, N, d_cp, 1, d_x, nnz, d_lib, d_f, d_ws, wsb, d_out);
      if (!rc) {
        io.down(cpm, d_out, sizeof(double) * (size_t)nnz);
        if (lib) io.down(lib, d_lib, sizeof(double) * (size_t)N);
      }
    }
    if (!io.ok() || rc) return io.drain(rc);
    return gficf_tmm_sync(ctx, d_ws);
  }
  io.up(d_row, rowidx, sizeof(int32_t) * (size_t)nnz);
  std::vector<double> h_sq, h_f75;
  if (!sq) { h_sq.resize((size_t)N); sq = h_sq.data(); }
  if (!f75) { h_f75.resize((size_t)N); f75 = h_f75.data(); }
  if (io.ok()) {
    rc = gficf_tmm_stats_device(ctx, G, N, d_cp, 1, d_row, d_x, nnz, max_cell, max_lds_n, d_ws, wsb, d_lib, d_sq, d_f75, d_os, d_gp);
    if (!rc) {
      io.down(lib, d_lib, sizeof(double) * (size_t)N);
      io.down(sq, d_sq, sizeof(double) * (size_t)N);
      io.down(f75, d_f75, sizeof(double) * (size_t)N);
      if (ostat) io.down(ostat, d_os, sizeof(double) * 2 * (size_t)N);
      io.down(gprime, d_gp, sizeof(int32_t));
    }
  }
  if (!io.ok() || rc) return io.drain(rc);
  rc = gficf_tmm_sync(ctx, d_ws);                          // the statistics are on the host, the input is checked
  if (rc) return rc;
  if (ref_col < 0) ref_col = tm_choose_ref(f75, sq, N);
  *ref_out = ref_col;
  rc = gficf_tmm_factors_device(ctx, G, N, d_cp, 1, d_row, d_x, nnz, max_cell, ref_col, d_lib, logratio_trim, sum_trim, do_weighting, max_lds_n, big_cells,
                                big_entries, 1, d_ws, wsb, d_f, d_n, d_kept);
  if (!rc) {
    io.down(factor, d_f, sizeof(double) * (size_t)N);
    if (n) io.down(n, d_n, sizeof(int32_t) * (size_t)N);
    if (kept) io.down(kept, d_kept, sizeof(int32_t) * (size_t)N);
  }
  if (!io.ok() || rc) return io.drain(rc);
  rc = gficf_tmm_sync(ctx, d_ws);
  if (rc) return rc;
  double sl = 0.0;
  for (int64_t c = 0; c < N; ++c) {
    if (factor_raw) factor_raw[c] = factor[c];
    sl += std::log(factor[c]);
  }
  const double gm = std::exp(sl / (double)N);
  for (int64_t c = 0; c < N; ++c) factor[c] = factor[c] / gm;
  if (!cpm) return GFICF_OK;
  io.up(d_f, factor, sizeof(double) * (size_t)N);
  if (io.ok()) {
    rc = gficf_tmm_cpm_device(ctx, N, d_cp, 1, d_x, nnz, d_lib, d_f, d_ws, wsb, d_out);
    if (!rc) io.down(cpm, d_out, sizeof(double) * (size_t)nnz);
  }
  if (!io.ok() || rc) return io.drain(rc);
  return gficf_tmm_sync(ctx, d_ws);
}

}  // extern "C"
