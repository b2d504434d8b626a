// pca_kernels.h — what pca.hip (libgficf_pca.so, the randomized SVD) and svds.hip (libgficf_svds.so, the exact truncated SVD)
// share as text: the CSC matrix with its segment table and Y = A'X, the rank-one centring, the Gram matrix, the one-workgroup
// eigen-solve, Y <- Y M, the sign rule, the layout conversion, and orth built from them.  include/gficf_pca.h states the
// arithmetic; pca.hip lists the launches.  Every includer gets its own copy (anonymous namespace), as with knn_tiles.h.
#pragma once

#include <cmath>

#include "common.h"

namespace {

constexpr int PCA_MAX_L = 128;             // GFICF_PCA_MAX_L of include/gficf_pca.h
constexpr int PCA_SEG = 1024;              // stored entries per (column, segment) unit
constexpr int PCA_CHUNKS = 256;            // chunks of rows of a Gram matrix / a column sum, at most
constexpr int PCA_EIG_T = 512;             // threads of the eigen-solve
constexpr int PCA_EIG_SWEEPS = 30;
constexpr int PCA_AP = PCA_MAX_L + 1;      // the Jacobi matrix's LDS block holds PCA_MAX_L rows of this pitch
constexpr double PCA_EPS = 2.220446049250313e-16;
constexpr uint32_t PCA_ST_CSC = 1u;        // a row index outside [0, nrows), a column pointer outside [0, nnz] or decreasing
constexpr uint32_t PCA_ST_VALUE = 2u;      // a NaN or infinite value in a sparse or dense input

inline int pca_ld(int l) { return (l + 7) & ~7; }
inline int pca_lp(int l) { return l <= 16 ? 16 : l <= 32 ? 32 : l <= 64 ? 64 : 128; }
inline double pca_tau(int64_t m) { return (double)(m > 1024 ? m : 1024) * PCA_EPS; }

unsigned pca_grid(int64_t n, int per_block = 256) {
  const int64_t b = gficf_ceil_div(n > 0 ? n : 1, per_block);
  return (unsigned)(b < 16384 ? b : 16384);
}

// ------------------------------------------------------------------------------------------------ layout conversion
__global__ __launch_bounds__(256) void k_pca_in(int64_t rows, int l, int ld, const double* __restrict__ in, double* __restrict__ out,
                                                uint32_t* __restrict__ status) {
  const int64_t total = rows * ld;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
    const int64_t r = q / ld;
    const int j = (int)(q % ld);
    double v = 0.0;
    if (j < l) {
      v = in[r + (int64_t)j * rows];
      if (!isfinite(v)) atomicOr(status, PCA_ST_VALUE);
    }
    out[q] = v;
  }
}

// out (rows x k, column-major) = in[:, 0 .. k) * sgn (sgn == nullptr: as it is)
__global__ __launch_bounds__(256) void k_pca_out(int64_t rows, int k, int ld, const double* __restrict__ in, const double* __restrict__ sgn,
                                                 double* __restrict__ out) {
  const int64_t total = rows * k;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
    const int64_t r = q % rows, j = q / rows;
    const double v = in[r * ld + j];
    out[q] = sgn ? v * sgn[j] : v;
  }
}

__global__ __launch_bounds__(256) void k_pca_copy(int64_t n, const double* __restrict__ in, double scale, int64_t stride, double* __restrict__ out) {
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (int64_t)gridDim.x * 256) out[q] = in[q * stride] * scale;
}

// rows x ld: column 0 = 1, the rest 0
__global__ __launch_bounds__(256) void k_pca_ones(int64_t rows, int ld, double* __restrict__ out) {
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < rows * ld; q += (int64_t)gridDim.x * 256) out[q] = (q % ld) == 0 ? 1.0 : 0.0;
}

// ------------------------------------------------------------------------------------------------ Y = A'X
struct PcaCsc {                 // a CSC matrix and its segment table
  int64_t nrows, ncols, nnz;
  const int64_t* colptr;
  const int32_t* rowidx;
  const double* x;
  int64_t* segptr;              // ncols + 1: first unit of every column, the number of units last
  int64_t max_units;            // what the partial rows have room for: ncols + nnz / PCA_SEG (every well-formed matrix fits)
};

inline int64_t pca_max_units(int64_t ncols, int64_t nnz) { return ncols + nnz / PCA_SEG + 1; }

__global__ __launch_bounds__(256) void k_pca_nseg(int64_t ncols, int64_t nnz, const int64_t* __restrict__ colptr, int64_t* __restrict__ seg,
                                                  uint32_t* __restrict__ status) {
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c <= ncols; c += (int64_t)gridDim.x * 256) {
    int64_t n = 0;
    if (c < ncols) {
      const int64_t b = colptr[c], e = colptr[c + 1];
      n = 1;
      if (b < 0 || e < b || e > nnz) atomicOr(status, PCA_ST_CSC);
      else if (e - b > PCA_SEG) n = gficf_ceil_div(e - b, PCA_SEG);
    }
    seg[c] = n;
  }
}

// GS lanes per group (one dense row per group and step), CPL columns per lane
template <int GS, int CPL>
__global__ __launch_bounds__(256) void k_pca_spmm(PcaCsc A, const double* __restrict__ X, int ld, double* __restrict__ out, double* __restrict__ part,
                                                  uint32_t* __restrict__ status) {
  constexpr int NG = 64 / GS;
  const int lane = threadIdx.x & 63, grp = lane / GS, j = lane % GS;
  const int64_t nw = ((int64_t)gridDim.x * 256) >> 6;
  int64_t total = A.segptr[A.ncols];
  if (total > A.max_units) total = A.max_units;               // (a malformed column pointer: flagged by k_pca_nseg)
  for (int64_t u = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6; u < total; u += nw) {
    int64_t lo = 0, hi = A.ncols - 1;                         // the last column whose first unit is <= u
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (A.segptr[mid] <= u) lo = mid; else hi = mid - 1;
    }
    const int64_t c = lo, s = u - A.segptr[c], nsg = A.segptr[c + 1] - A.segptr[c];
    int64_t b0 = A.colptr[c], e0 = A.colptr[c + 1];
    if (b0 < 0 || e0 < b0 || e0 > A.nnz) b0 = e0 = 0;
    const int64_t b = b0 + s * PCA_SEG < e0 ? b0 + s * PCA_SEG : e0, e = b + PCA_SEG < e0 ? b + PCA_SEG : e0;
    double acc[CPL];
#pragma unroll
    for (int cc = 0; cc < CPL; ++cc) acc[cc] = 0.0;
    for (int64_t p = b; p < e; p += 64) {
      int32_t r = 0;
      double v = 0.0;
      if (p + lane < e) {
        r = A.rowidx[p + lane];
        v = A.x[p + lane];
        if (!isfinite(v)) atomicOr(status, PCA_ST_VALUE);
        if (r < 0 || r >= A.nrows) { atomicOr(status, PCA_ST_CSC); r = 0; v = 0.0; }
      }
      const int cnt = e - p < 64 ? (int)(e - p) : 64;         // (entries past the end: value 0, row 0)
      for (int t = 0; t < cnt; t += 4 * NG) {                 // four dense rows in flight per group
        double xv[4][CPL], vv[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          const int32_t rr = __shfl(r, t + f * NG + grp);
          vv[f] = __shfl(v, t + f * NG + grp);
          const double* row = X + (int64_t)rr * ld;
#pragma unroll
          for (int cc = 0; cc < CPL; ++cc) xv[f][cc] = j + cc * 64 < ld ? row[j + cc * 64] : 0.0;
        }
#pragma unroll
        for (int f = 0; f < 4; ++f)
#pragma unroll
          for (int cc = 0; cc < CPL; ++cc) acc[cc] = fma(vv[f], xv[f][cc], acc[cc]);
      }
    }
#pragma unroll
    for (int cc = 0; cc < CPL; ++cc)
#pragma unroll
      for (int d = 32; d >= GS; d >>= 1) acc[cc] += __shfl_xor(acc[cc], d);
    double* dst = nsg == 1 ? out + c * ld : part + u * ld;
    if (grp == 0)
#pragma unroll
      for (int cc = 0; cc < CPL; ++cc)
        if (j + cc * 64 < ld) dst[j + cc * 64] = acc[cc];
  }
}

// one wave per column of several segments
__global__ __launch_bounds__(256) void k_pca_spmm_sum(int64_t ncols, const int64_t* __restrict__ segptr, int64_t max_units, const double* __restrict__ part,
                                                      int ld, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  for (int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6; c < ncols; c += ((int64_t)gridDim.x * 256) >> 6) {
    const int64_t u0 = segptr[c];
    int64_t u1 = segptr[c + 1];
    if (u1 - u0 < 2) continue;
    if (u1 > max_units) u1 = max_units;
    for (int col = lane; col < ld; col += 64) {
      double s = 0.0;
      for (int64_t u = u0; u < u1; ++u) s += part[u * ld + col];
      out[c * ld + col] = s;
    }
  }
}

int pca_csc_prepare(gficf_ctx* ctx, const PcaCsc& A, uint32_t* status) {
  hipLaunchKernelGGL(k_pca_nseg, dim3(pca_grid(A.ncols + 1)), dim3(256), 0, ctx->stream, A.ncols, A.nnz, A.colptr, A.segptr, status);
  GFICF_HIP_CHECK(hipGetLastError());
  return gficf_exclusive_scan_i64(ctx, A.segptr, A.ncols + 1);
}

// out (ncols x ld) = A' X (X: nrows x ld); part: max_units x ld
int pca_spmm(gficf_ctx* ctx, const PcaCsc& A, const double* X, int l, double* out, double* part, uint32_t* status) {
  const int ld = pca_ld(l);
  const dim3 grid(pca_grid(A.max_units, 4)), blk(256);
  hipStream_t st = ctx->stream;
  if (l <= 8) hipLaunchKernelGGL((k_pca_spmm<8, 1>), grid, blk, 0, st, A, X, ld, out, part, status);
  else if (l <= 16) hipLaunchKernelGGL((k_pca_spmm<16, 1>), grid, blk, 0, st, A, X, ld, out, part, status);
  else if (l <= 32) hipLaunchKernelGGL((k_pca_spmm<32, 1>), grid, blk, 0, st, A, X, ld, out, part, status);
  else if (l <= 64) hipLaunchKernelGGL((k_pca_spmm<64, 1>), grid, blk, 0, st, A, X, ld, out, part, status);
  else hipLaunchKernelGGL((k_pca_spmm<64, 2>), grid, blk, 0, st, A, X, ld, out, part, status);
  hipLaunchKernelGGL(k_pca_spmm_sum, dim3(pca_grid(A.ncols, 4)), blk, 0, st, A.ncols, (const int64_t*)A.segptr, A.max_units, (const double*)part, ld, out);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

// ------------------------------------------------------------------------------------------------ w'X and Y -= a v'
inline int64_t pca_chunks(int64_t m) { const int64_t c = gficf_ceil_div(m > 0 ? m : 1, 256); return c < PCA_CHUNKS ? c : PCA_CHUNKS; }

__global__ __launch_bounds__(256) void k_pca_colsum(const double* __restrict__ X, int64_t m, int ld, const double* __restrict__ w, int64_t rpc,
                                                    double* __restrict__ cpart) {
  __shared__ double s[4][PCA_MAX_L];
  const int lane = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * rpc, r1 = r0 + rpc < m ? r0 + rpc : m;
  double acc[2] = {0.0, 0.0};
  for (int64_t r = r0 + rl; r < r1; r += 4) {
    const double a = w ? w[r] : 1.0;
#pragma unroll
    for (int cc = 0; cc < 2; ++cc)
      if (lane + cc * 64 < ld) acc[cc] = fma(a, X[r * ld + lane + cc * 64], acc[cc]);
  }
  s[rl][lane] = acc[0];
  s[rl][lane + 64] = acc[1];
  __syncthreads();
  if (rl == 0)
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      const int col = lane + cc * 64;
      cpart[(int64_t)blockIdx.x * PCA_MAX_L + col] = ((s[0][col] + s[1][col]) + s[2][col]) + s[3][col];
    }
}

__global__ __launch_bounds__(PCA_MAX_L) void k_pca_colsum_fin(const double* __restrict__ cpart, int nch, double* __restrict__ vec) {
  double s = 0.0;
  for (int ch = 0; ch < nch; ++ch) s += cpart[(int64_t)ch * PCA_MAX_L + threadIdx.x];
  vec[threadIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_pca_rank1(double* __restrict__ Y, int64_t m, int ld, const double* __restrict__ a, const double* __restrict__ vec) {
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < m * ld; q += (int64_t)gridDim.x * 256) {
    const int64_t r = q / ld;
    Y[q] -= (a ? a[r] : 1.0) * vec[q % ld];
  }
}

// Y (my x ld) -= a (or 1) * (w (or 1)' X), X: mx x ld
int pca_centre(gficf_ctx* ctx, const double* X, int64_t mx, const double* w, double* Y, int64_t my, const double* a, int ld, double* cpart, double* cvec) {
  const int64_t nch = pca_chunks(mx), rpc = gficf_ceil_div(mx, nch);
  hipLaunchKernelGGL(k_pca_colsum, dim3((unsigned)nch), dim3(256), 0, ctx->stream, X, mx, ld, w, rpc, cpart);
  hipLaunchKernelGGL(k_pca_colsum_fin, dim3(1), dim3(PCA_MAX_L), 0, ctx->stream, (const double*)cpart, (int)nch, cvec);
  hipLaunchKernelGGL(k_pca_rank1, dim3(pca_grid(my * ld)), dim3(256), 0, ctx->stream, Y, my, ld, a, (const double*)cvec);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

// ------------------------------------------------------------------------------------------------ Gram matrix
// thread (tx, ty) of 16 x 16 holds S[tx + 16 a][ty + 16 b]; rows staged 16 at a time
template <int NB>
__global__ __launch_bounds__(256) void k_pca_gram(const double* __restrict__ Y, int64_t m, int ld, int64_t rpc, double* __restrict__ gpart) {
  constexpr int LP = NB * 16;
  __shared__ double sY[16][LP];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * rpc, r1 = r0 + rpc < m ? r0 + rpc : m;
  double acc[NB][NB];
#pragma unroll
  for (int a = 0; a < NB; ++a)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[a][b] = 0.0;
  for (int64_t t0 = r0; t0 < r1; t0 += 16) {
    for (int q = threadIdx.x; q < 16 * LP; q += 256) {
      const int rr = q / LP, cc = q % LP;
      sY[rr][cc] = (t0 + rr < r1 && cc < ld) ? Y[(t0 + rr) * ld + cc] : 0.0;
    }
    __syncthreads();
#pragma unroll 4
    for (int rr = 0; rr < 16; ++rr) {
      double ya[NB], yb[NB];
#pragma unroll
      for (int a = 0; a < NB; ++a) { ya[a] = sY[rr][tx + 16 * a]; yb[a] = sY[rr][ty + 16 * a]; }
#pragma unroll
      for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[a][b] = fma(ya[a], yb[b], acc[a][b]);
    }
    __syncthreads();
  }
  double* dst = gpart + (int64_t)blockIdx.x * LP * LP;
#pragma unroll
  for (int a = 0; a < NB; ++a)
#pragma unroll
    for (int b = 0; b < NB; ++b) dst[(tx + 16 * a) * LP + ty + 16 * b] = acc[a][b];
}

__global__ __launch_bounds__(256) void k_pca_gram_fin(const double* __restrict__ gpart, int nch, int n, double* __restrict__ S) {
  for (int q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) {
    double s = 0.0;
    for (int ch = 0; ch < nch; ++ch) s += gpart[(int64_t)ch * n + q];
    S[q] = s;
  }
}

// ------------------------------------------------------------------------------------------------ eigen-solve
// S (l x l, pitch LP, symmetric) = W diag(lam) W'.  Parallel cyclic Jacobi: the round-robin schedule gives le / 2 disjoint pairs
// per step (le = l rounded up to even; the extra index is a zero row), every pair's rotation is computed from the matrix as the
// step finds it, then every 2 x 2 block (pair of rows, pair of columns) is rotated from both sides by one thread, and the vectors'
// column pairs from the right (two barriers per step).  A pair is left
// alone when |a_pq| <= eps * max(sqrt(|a_pp a_qq|), tau * max|a_ii|): below that it moves neither a kept value nor a kept
// vector by more than a rounding error.  The sweeps end when one rotates nothing (or after PCA_EIG_SWEEPS).
// Out, sorted by decreasing lam, a direction with lam <= tau * lam_max dropped (zero column, d = 0):
//   dv = sqrt(lam);  Minv = W diag(1 / dv);  Mfwd = W diag(dv);  Mkeep = W.
__global__ __launch_bounds__(PCA_EIG_T) void k_pca_eig(const double* __restrict__ S, int LP, int l, double tau, double* __restrict__ V,
                                                       double* __restrict__ Minv, double* __restrict__ Mfwd, double* __restrict__ Mkeep, double* __restrict__ dv) {
  __shared__ double sA[PCA_MAX_L * PCA_AP];
  __shared__ double sC[PCA_MAX_L / 2], sS[PCA_MAX_L / 2], sLam[PCA_MAX_L];
  __shared__ int sP[PCA_MAX_L / 2], sQ[PCA_MAX_L / 2], sOrd[PCA_MAX_L];
  __shared__ double sMax;
  const int tid = threadIdx.x, le = (l + 1) & ~1, hp = le / 2, pa = le + 1;       // (pa odd: a column walk hits every bank)
  // the vectors sit in LDS behind the matrix while both fit (l <= 90), in global memory beyond
  const bool v_lds = 2 * le * pa <= PCA_MAX_L * PCA_AP;
  double* const Vw = v_lds ? sA + le * pa : V;
  const int pv = v_lds ? pa : LP;
  for (int q = tid; q < le * le; q += PCA_EIG_T) {
    const int i = q / le, j = q % le;
    sA[i * pa + j] = (i < l && j < l) ? S[i * LP + j] : 0.0;
    Vw[i * pv + j] = i == j ? 1.0 : 0.0;
  }
  __syncthreads();
  if (tid == 0) {
    double mx = 0.0;
    for (int i = 0; i < l; ++i) mx = fmax(mx, fabs(sA[i * pa + i]));
    sMax = mx;
  }
  __syncthreads();
  const double floor_abs = PCA_EPS * tau * sMax;
  for (int sweep = 0; sweep < PCA_EIG_SWEEPS; ++sweep) {
    int rotated = 0;
    for (int step = 0; step < le - 1; ++step) {
      if (tid < hp) {
        const int p = tid == 0 ? le - 1 : (step + tid) % (le - 1), q = tid == 0 ? step : (step - tid + le - 1) % (le - 1);
        const double app = sA[p * pa + p], aqq = sA[q * pa + q], apq = sA[p * pa + q];
        double c = 1.0, s = 0.0;
        if (fabs(apq) > fmax(PCA_EPS * sqrt(fabs(app * aqq)), floor_abs)) {
          const double th = (aqq - app) / (2.0 * apq);
          const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(1.0 + th * th));
          c = 1.0 / sqrt(1.0 + t * t);
          s = t * c;
          rotated = 1;
        }
        sP[tid] = p; sQ[tid] = q; sC[tid] = c; sS[tid] = s;
      }
      __syncthreads();
      for (int it = tid; it < hp * hp; it += PCA_EIG_T) {       // A <- J' A J, block (pair bi of rows, pair bj of columns)
        const int bi = it / hp, bj = it % hp;
        const int p1 = sP[bi], q1 = sQ[bi], p2 = sP[bj], q2 = sQ[bj];
        const double ci = sC[bi], si = sS[bi], cj = sC[bj], sj = sS[bj];
        if (si == 0.0 && sj == 0.0) continue;
        const double a = sA[p1 * pa + p2], b = sA[p1 * pa + q2], c = sA[q1 * pa + p2], d = sA[q1 * pa + q2];
        const double ra = ci * a - si * c, rb = ci * b - si * d, rc = si * a + ci * c, rd = si * b + ci * d;
        const bool diag = bi == bj;
        sA[p1 * pa + p2] = cj * ra - sj * rb;
        sA[p1 * pa + q2] = diag ? 0.0 : sj * ra + cj * rb;
        sA[q1 * pa + p2] = diag ? 0.0 : cj * rc - sj * rd;
        sA[q1 * pa + q2] = sj * rc + cj * rd;
      }
      for (int it = tid; it < le * hp; it += PCA_EIG_T) {       // V <- V J
        const int i = it / hp, bj = it % hp;
        const double cj = sC[bj], sj = sS[bj];
        if (sj == 0.0) continue;
        const int p2 = sP[bj], q2 = sQ[bj];
        const double vp = Vw[i * pv + p2], vq = Vw[i * pv + q2];
        Vw[i * pv + p2] = cj * vp - sj * vq;
        Vw[i * pv + q2] = sj * vp + cj * vq;
      }
      __syncthreads();
    }
    if (!__syncthreads_or(rotated)) break;
  }
  if (tid < l) sLam[tid] = sA[tid * pa + tid];
  __syncthreads();
  if (tid < l) {
    const double me = sLam[tid];
    int r = 0;
    for (int j = 0; j < l; ++j) r += (sLam[j] > me || (sLam[j] == me && j < tid)) ? 1 : 0;
    sOrd[tid] = r < l ? r : l - 1;
  }
  if (tid == 0) {
    double mx = 0.0;
    for (int i = 0; i < l; ++i) mx = fmax(mx, sLam[i]);
    sMax = mx;
  }
  for (int q = tid; q < LP * LP; q += PCA_EIG_T)            // the padding; every (i, r) below l is written once further down
    if (q / LP >= l || q % LP >= l) { Minv[q] = 0.0; Mfwd[q] = 0.0; Mkeep[q] = 0.0; }
  for (int q = l + tid; q < LP; q += PCA_EIG_T) dv[q] = 0.0;
  __syncthreads();
  const double thr = tau * sMax;
  for (int q = tid; q < l * l; q += PCA_EIG_T) {
    const int i = q / l, c = q % l, r = sOrd[c];
    const double lam = sLam[c];
    const bool keep = lam > thr && lam > 0.0;
    const double dd = keep ? sqrt(lam) : 0.0, v = Vw[i * pv + c];
    Minv[i * LP + r] = keep ? v / dd : 0.0;
    Mfwd[i * LP + r] = keep ? v * dd : 0.0;
    Mkeep[i * LP + r] = keep ? v : 0.0;
    if (i == 0) dv[r] = dd;
  }
}

// ------------------------------------------------------------------------------------------------ Y <- Y M
// a wave takes 8 rows at a time: the rows in LDS, a row of M per step from L2 (the same for every wave), lanes on the columns
template <int CPL>
__global__ __launch_bounds__(256) void k_pca_apply(const double* __restrict__ Yin, int64_t m, int ld, int l, const double* __restrict__ M, int LP,
                                                   double* __restrict__ Yout) {
  __shared__ double sRow[4][8][PCA_MAX_L];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int64_t r0 = ((int64_t)blockIdx.x * 4 + wv) * 8; r0 < m; r0 += (int64_t)gridDim.x * 32) {
#pragma unroll
    for (int rr = 0; rr < 8; ++rr)
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) {
        const int col = lane + cc * 64;
        sRow[wv][rr][col] = (r0 + rr < m && col < ld) ? Yin[(r0 + rr) * ld + col] : 0.0;
      }
    GFICF_WAVE_SYNC();
    double acc[8][CPL];
#pragma unroll
    for (int rr = 0; rr < 8; ++rr)
#pragma unroll
      for (int cc = 0; cc < CPL; ++cc) acc[rr][cc] = 0.0;
    for (int i = 0; i < l; ++i) {
      double mv[CPL];
#pragma unroll
      for (int cc = 0; cc < CPL; ++cc) mv[cc] = lane + cc * 64 < LP ? M[i * LP + lane + cc * 64] : 0.0;
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) {
        const double a = sRow[wv][rr][i];
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) acc[rr][cc] = fma(a, mv[cc], acc[rr][cc]);
      }
    }
#pragma unroll
    for (int rr = 0; rr < 8; ++rr)
#pragma unroll
      for (int cc = 0; cc < CPL; ++cc)
        if (r0 + rr < m && lane + cc * 64 < ld) Yout[(r0 + rr) * ld + lane + cc * 64] = acc[rr][cc];
    GFICF_WAVE_SYNC();
  }
}

// ------------------------------------------------------------------------------------------------ sign rule
// one workgroup per component: +1 or -1 so that the first entry of largest magnitude of column j is positive
__global__ __launch_bounds__(256) void k_pca_sign(const double* __restrict__ genes, int64_t rows, int ld, double* __restrict__ sgn) {
  __shared__ double sAbs[256], sVal[256];
  __shared__ int64_t sIdx[256];
  const int j = blockIdx.x;
  double best = -1.0, val = 0.0;
  int64_t idx = rows;
  for (int64_t r = threadIdx.x; r < rows; r += 256) {
    const double v = genes[r * ld + j];
    if (fabs(v) > best) { best = fabs(v); val = v; idx = r; }
  }
  sAbs[threadIdx.x] = best; sVal[threadIdx.x] = val; sIdx[threadIdx.x] = idx;
  __syncthreads();
  for (int d = 128; d >= 1; d >>= 1) {
    if (threadIdx.x < d) {
      const int o = threadIdx.x + d;
      if (sAbs[o] > sAbs[threadIdx.x] || (sAbs[o] == sAbs[threadIdx.x] && sIdx[o] < sIdx[threadIdx.x])) {
        sAbs[threadIdx.x] = sAbs[o]; sVal[threadIdx.x] = sVal[o]; sIdx[threadIdx.x] = sIdx[o];
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) sgn[j] = sVal[0] < 0.0 ? -1.0 : 1.0;
}

// ------------------------------------------------------------------------------------------------ the small matrices, orth
struct PcaSmall {
  double *gpart, *S, *V, *Minv, *Mfwd, *Mkeep, *dv, *cpart, *cvec, *sgn;
};

void pca_carve_small(gficf_carver& cv, int64_t m_max, int l, PcaSmall& s) {
  const size_t lp = (size_t)pca_lp(l), lp2 = lp * lp;
  s.gpart = cv.take<double>((size_t)pca_chunks(m_max) * lp2);
  s.S = cv.take<double>(lp2);
  s.V = cv.take<double>(lp2);
  s.Minv = cv.take<double>(lp2);
  s.Mfwd = cv.take<double>(lp2);
  s.Mkeep = cv.take<double>(lp2);
  s.dv = cv.take<double>(lp);
  s.cpart = cv.take<double>((size_t)PCA_CHUNKS * PCA_MAX_L);
  s.cvec = cv.take<double>(PCA_MAX_L);
  s.sgn = cv.take<double>(PCA_MAX_L);
}

// the Gram matrix of Y (m x ld) and its eigen-solve: s.Minv / s.Mfwd / s.Mkeep / s.dv
int pca_gram_eig(gficf_ctx* ctx, const PcaSmall& s, const double* Y, int64_t m, int l) {
  const int ld = pca_ld(l), lp = pca_lp(l);
  const int64_t nch = pca_chunks(m), rpc = gficf_ceil_div(m, nch);
  hipStream_t st = ctx->stream;
  const dim3 grid((unsigned)nch), blk(256);
  if (lp == 16) hipLaunchKernelGGL(k_pca_gram<1>, grid, blk, 0, st, Y, m, ld, rpc, s.gpart);
  else if (lp == 32) hipLaunchKernelGGL(k_pca_gram<2>, grid, blk, 0, st, Y, m, ld, rpc, s.gpart);
  else if (lp == 64) hipLaunchKernelGGL(k_pca_gram<4>, grid, blk, 0, st, Y, m, ld, rpc, s.gpart);
  else hipLaunchKernelGGL(k_pca_gram<8>, grid, blk, 0, st, Y, m, ld, rpc, s.gpart);
  hipLaunchKernelGGL(k_pca_gram_fin, dim3(pca_grid(lp * lp)), blk, 0, st, (const double*)s.gpart, (int)nch, lp * lp, s.S);
  hipLaunchKernelGGL(k_pca_eig, dim3(1), dim3(PCA_EIG_T), 0, st, (const double*)s.S, lp, l, pca_tau(m), s.V, s.Minv, s.Mfwd, s.Mkeep, s.dv);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int pca_apply(gficf_ctx* ctx, const double* Yin, int64_t m, int l, const double* M, double* Yout) {
  const int ld = pca_ld(l), lp = pca_lp(l);
  const dim3 grid(pca_grid(m, 32)), blk(256);
  if (lp <= 64) hipLaunchKernelGGL(k_pca_apply<1>, grid, blk, 0, ctx->stream, Yin, m, ld, l, M, lp, Yout);
  else hipLaunchKernelGGL(k_pca_apply<2>, grid, blk, 0, ctx->stream, Yin, m, ld, l, M, lp, Yout);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

// orth, twice: the result is back in `cur` (`other`: scratch of the same size)
int pca_orth(gficf_ctx* ctx, const PcaSmall& s, double* cur, double* other, int64_t m, int l) {
  int rc = pca_gram_eig(ctx, s, cur, m, l);
  if (!rc) rc = pca_apply(ctx, cur, m, l, s.Minv, other);
  if (!rc) rc = pca_gram_eig(ctx, s, other, m, l);
  if (!rc) rc = pca_apply(ctx, other, m, l, s.Minv, cur);
  return rc;
}

}  // namespace
